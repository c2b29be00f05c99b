"""The pure host parts of hit attribution (pointvs_amd/hit_attribution.py, screening.slot_offsets) that the four
attribution methods of ScreeningSweep share: slot offsets, hit validation, the split of copy rows into scores, the
column check and the label lists of the three line formats. CPU tensors only: no GPU, no library."""
import pytest
import torch

from pointvs_amd import hit_attribution as HA
from pointvs_amd.screening import MAX_SCREEN_LIGAND_ATOMS, slot_offsets


def test_slot_offsets_are_rowwise_prefix_sums_with_empty_trailing_slots():
    ptrs = slot_offsets([[5, 1, 12], [7]], 3)
    assert ptrs.dtype == torch.int32
    assert ptrs.tolist() == [[0, 5, 6, 18], [0, 7, 7, 7]]      # (the empty slots repeat the last offset)
    one_empty = slot_offsets([[]], 3)
    assert one_empty.dtype == torch.int32 and one_empty.tolist() == [[0, 0, 0, 0]]
    none = slot_offsets([], 3)
    assert none.dtype == torch.int32 and tuple(none.shape) == (0, 4)


def _hit(name, n, n_feats=4):
    return name, torch.zeros(n, n_feats), torch.zeros(n, 3)


@pytest.mark.parametrize('who', ['ligand_atom_masking', 'receptor_hotspots'])
def test_hit_validation_refuses_with_the_callers_name(who):
    wide = MAX_SCREEN_LIGAND_ATOMS + 1
    bad = {
        'names must be unique': [_hit('a', 3), _hit('b', 2), _hit('a', 5)],
        f"ligand 'big' has {wide} atoms": [_hit('a', 3), _hit('big', wide)],
        "ligand 'flat': lig_feats [n, F] and ONE pose [n, 3]": [('flat', torch.zeros(3, 4), torch.zeros(3, 2))],
        "ligand 'rows': lig_feats [n, F] and ONE pose [n, 3]": [('rows', torch.zeros(4, 4), torch.zeros(3, 3))],
    }
    for text, items in bad.items():
        with pytest.raises(ValueError) as err:
            HA.Hits(iter(items), who)
        assert str(err.value).startswith(who + ': ') and text in str(err.value)


def test_hits_record_and_its_one_packing():
    items = [_hit('a', 3), _hit('none', 0), _hit('b', 2)]
    items[2][2][1, 0] = 7.0
    hits = HA.Hits(iter(items), 'contact_masking')
    assert hits.names == ['a', 'none', 'b'] and hits.ns == [3, 0, 2] and hits.pos is None
    packed = hits.pack(torch.device('cpu'))
    assert packed is hits and hits.lig_ptr.dtype == torch.int32 and hits.lig_ptr.tolist() == [0, 3, 3, 5]
    assert tuple(hits.pos.shape) == (5, 3) and tuple(hits.feats.shape) == (5, 4) and hits.pos[4, 0] == 7.0
    pos = hits.pos
    assert hits.pack(torch.device('cpu')).pos is pos      # (packed once)
    empty = HA.Hits([], 'contact_masking')
    assert empty.items == [] and empty.names == [] and empty.ns == []


def test_score_split_equals_a_per_hit_loop():
    names, counts = ['none', 'one', 'four'], [0, 1, 4]
    torch.manual_seed(11)
    raw = torch.randn(sum(counts) + len(counts), 3)
    scored = torch.sigmoid(raw)
    for column in range(3):
        raws, scores = HA.split_scores(names, counts, raw, scored, column)
        at = 0
        for name, k in zip(names, counts):       # hit s: one row for the whole complex, then counts[s] copies
            assert torch.equal(raws[name], raw[at:at + k + 1])
            expect = torch.stack([scored[at, column] - scored[at + 1 + i, column] for i in range(k)]) if k \
                else torch.empty(0)
            assert scores[name].shape == (k,) and torch.equal(scores[name], expect)
            at += k + 1
        assert at == raw.shape[0]
    assert scores['none'].numel() == 0 and raws['none'].shape == (1, 3)      # K = 0: empty, and one row consumed
    assert torch.equal(raws['one'][0], raw[1])


@pytest.mark.parametrize('who', ['ligand_atom_masking', 'contact_masking', 'receptor_atom_masking'])
def test_column_check(who):
    n_outputs = 3
    for column in range(n_outputs):
        assert HA.checked_column(who, column, n_outputs) == column
    for column in (-1, n_outputs):
        with pytest.raises(ValueError) as err:
            HA.checked_column(who, column, n_outputs)
        assert str(err.value) == f'{who}: column {column} of 3 outputs'


def test_label_lists_of_the_three_line_formats():
    names = ['x', 'none', 'yz']
    assert HA.ligand_atom_labels(names, [2, 0, 3]) == ['x_atom0', 'x_atom1', 'yz_atom0', 'yz_atom1', 'yz_atom2']
    assert HA.contact_labels(names, [2, 0, 1], [[0, 41], [1, 7], [2, 7]]) == \
        ['x_atom0 atom41', 'x_atom1 atom7', 'yz_atom2 atom7']
    assert HA.receptor_atom_labels(names, [1, 0, 2], [5, 5, 9]) == ['x atom5', 'yz atom5', 'yz atom9']
    assert HA.ligand_atom_labels([], []) == [] and HA.contact_labels([], [], []) == []
    assert HA.receptor_atom_labels(names, [0, 0, 0], []) == []
