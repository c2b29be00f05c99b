"""The three routes of a LibraryScreen (pointvs_amd/library_steps.py) on the device: every screen reports the route
that `library_route` picked, and after one eager step `_fast` holds exactly the buffer set the route declares - written
down here as literals, from the buffer sets the screen allocated before the steps were classes. The small shape of
tools/launch_sequence.py --screening: a 130-atom receptor, a batch of 3, slots of 7 / 20 / 3 atoms, edge radius 7, two
layers."""
import pytest
import torch

from tests.test_gpu_screen_crop import _model, _set

pytestmark = pytest.mark.gpu

SIZES, RADIUS = (7, 20, 3), 7.0
BUILDER = {'cap', 'cap_l', 'status', 'ones', 'state', 'node_ptr', 'node_graph', 'pos', 'x', 'inv_deg'}
FULL = {'rowptr', 'row', 'col', 'etype'}
REUSE = BUILDER | FULL | {k + '_l' for k in FULL} | {'base_magg', 'base_xsum', 'base_deg', 'pgs'}
CROPPED = BUILDER | FULL | {'keep', 'pg'}


@pytest.fixture(scope='module')
def case():
    from pointvs_amd.synthetic import random_poses
    lig, rec, lig_feats, rec_feats = _set(6006, n_lig=20)
    slots = [(lig_feats[:n].roll(k, 0).contiguous(), random_poses(lig[:n], 1, seed=90 + k, max_shift=3.0)[0])
             for k, n in enumerate(SIZES)]
    return rec.cuda(), rec_feats, slots


def _stepped(case, model, rec_drop=None, **kw):
    from pointvs_amd.screening import LibraryScreen
    rec, rec_feats, slots = case
    screen = LibraryScreen(model, rec, rec_feats, len(SIZES), 20, RADIUS, **kw)
    y = screen.load(slots, rec_drop=rec_drop)()
    screen.check()
    assert y.shape[0] == len(SIZES) and bool(torch.isfinite(y).all())
    return screen


def test_reuse(case):
    screen = _stepped(case, _model(1))
    f = screen._fast
    assert screen.route == 'reuse' and screen.reuse is True and screen.capture_refusal() is None
    assert set(f) == REUSE and f['cap_l'] is not None and set(f['pgs']) == {screen.n_cap}
    assert screen.rec_drop is None and screen.contact is None and screen.cam is None and not screen.needs_sizing_batch()
    with pytest.raises(RuntimeError, match='keep: the masks of a cropped screen'):
        screen.keep


def test_reuse_with_contact_attention(case):
    attending = _model(2, edge_attention=True)
    first = _stepped(case, attending, contact_attention=1)
    assert first.route == 'reuse' and set(first._fast) == REUSE | {'att_l'}
    assert bool((first.contact['rec_count'] > 0).any())
    last = _stepped(case, attending, contact_attention=-1)
    assert last.route == 'reuse' and last.contact_attention == 2 and set(last._fast) == REUSE
    assert bool((last.contact['rec_count'] > 0).any())


def test_reuse_with_struck_slots(case):
    screen = _stepped(case, _model(1), rec_drop=[-1, 5, 77], struck=True)
    assert screen.route == 'reuse' and set(screen._fast) == REUSE
    assert screen.rec_drop is not None and screen.rec_drop.tolist() == [-1, 5, 77]
    assert int(screen._fast['node_ptr'][3]) == sum(SIZES) + 3 * 130 - 2


def test_reuse_with_cam(case):
    screen = _stepped(case, _model(1), cam=True)
    assert screen.route == 'reuse' and set(screen._fast) == REUSE
    assert bool(torch.isfinite(screen.cam['slot_rec_val']).all()) and bool((screen.cam['rec_count'] == 3).all())


def test_cropped(case):
    screen = _stepped(case, _model(1), crop_radius=6.0)
    f = screen._fast
    assert screen.route == 'cropped' and screen.reuse is True and screen.capture_refusal() is None
    assert set(f) == CROPPED and f['cap_l'] is None and screen.keep is f['keep']
    assert not any(k.endswith('_l') and k != 'cap_l' for k in f) and not any(k.startswith('base_') for k in f)
    assert screen.rec_drop is None and not hasattr(screen, 'crop_pos') and not hasattr(screen, 'rec_magg')


def test_cropped_with_crop_parents(case):
    plain = _stepped(case, _model(1), crop_radius=6.0)
    screen = _stepped(case, _model(1), crop_radius=6.0, crop_parents=True)
    assert screen.route == 'cropped' and set(screen._fast) == CROPPED and screen._fast['cap_l'] is None
    assert screen.crop_pos.shape == (60, 3) and torch.equal(screen.crop_ptr, screen.lig_ptr)
    assert screen.rec_drop.tolist() == [-1, -1, -1] and torch.equal(screen.keep, plain.keep)


def test_cropped_with_cropped_maps_and_cam(case):
    screen = _stepped(case, _model(1), crop_radius=6.0, cropped_maps=True, cam=True)
    assert screen.route == 'cropped' and set(screen._fast) == CROPPED
    val, count = screen.cam['slot_rec_val'], screen.cam['rec_count']
    assert bool(torch.isfinite(val).any()) and bool(torch.isnan(val).any())      # (kept atoms have a value, others NaN)
    assert 0 < int(count.max()) <= 3 and int(count.sum()) == int(torch.isfinite(val).sum())


def test_cropped_with_cropped_maps_and_contact_attention(case):
    screen = _stepped(case, _model(2, edge_attention=True), crop_radius=6.0, cropped_maps=True, contact_attention=1)
    assert screen.route == 'cropped' and set(screen._fast) == CROPPED
    assert bool((screen.contact['rec_count'] > 0).any())


def test_plain(case):
    screen = _stepped(case, _model(1, k=16))
    assert screen.route == 'plain' and screen.reuse is False and screen._fast is None
    assert not screen.needs_sizing_batch() and not screen.stale()
    assert screen.capture_refusal().startswith('capture needs the first-layer reuse')
    with pytest.raises(RuntimeError, match='capture needs the first-layer reuse'):
        screen.capture()
    with_cam = _stepped(case, _model(1, k=16), cam=True)
    assert with_cam.route == 'plain' and with_cam._fast is None
    assert bool(torch.isfinite(with_cam.cam['slot_rec_val']).all())
