"""The route of a LibraryScreen (pointvs_amd/library_steps.py), the host side (CPU): `library_route` / `model_route`
through the table of models and keywords, and the steps' capture refusals in their present words."""
from types import SimpleNamespace

import pytest

from tests.test_gpu_screen_crop import _model

SOFT = dict(edge_attention=True, softmax_attention=True)

# (model flags, softmax_reuse, the uncropped route)
TABLE = [
    (dict(k=32), False, 'reuse'),
    (dict(k=64), False, 'reuse'),
    (dict(k=32, edge_attention=True, node_attention=True, graphnorm=True, residual=True), False, 'reuse'),
    (dict(k=16), False, 'plain'),
    (dict(k=128), False, 'plain'),
    (dict(k=32, edge_residual=True), False, 'plain'),
    (dict(k=64, edge_residual=True), True, 'plain'),
    (dict(k=32, **SOFT), False, 'plain'),
    (dict(k=32, **SOFT), True, 'reuse'),
    (dict(k=64, **SOFT), True, 'reuse'),
    (dict(k=48, **SOFT), True, 'plain'),
    (dict(k=32, softmax_attention=True), True, 'plain'),
    (dict(k=32, softmax_attention=True), False, 'plain'),
    (dict(k=32, edge_residual=True, **SOFT), True, 'plain'),
]


@pytest.mark.parametrize('flags,softmax_reuse,want', TABLE, ids=[f'{i}-{row[2]}' for i, row in enumerate(TABLE)])
def test_the_route_of_every_row(flags, softmax_reuse, want):
    from pointvs_amd.captured_scoring import model_refusal
    from pointvs_amd.screening import library_route, model_route
    model = _model(**flags)
    assert model_route(model, softmax_reuse=softmax_reuse) == want
    first = model.layers[1]
    facts = (first.hidden_nf, any(l.edge_residual for l in list(model.layers)[1:]), first.softmax_attention,
             first.edge_attention)
    assert facts[0] == flags['k'] and library_route(*facts, softmax_reuse=softmax_reuse) == want
    # crop_radius selects the cropped route for every model that a cropped screen accepts, whatever the row says
    if model_refusal(model) is None:
        assert model_route(model, softmax_reuse=softmax_reuse, crop_radius=6.0) == 'cropped'
        assert library_route(*facts, softmax_reuse=softmax_reuse, crop_radius=6.0) == 'cropped'


def test_the_table_has_accepted_and_refused_models_under_the_crop():
    from pointvs_amd.captured_scoring import model_refusal
    refused = [model_refusal(_model(**flags)) is not None for flags, _, _ in TABLE]
    assert any(refused) and not all(refused)
    assert refused[3] and refused[5] and not refused[0] and not refused[4] and not refused[8]


def test_a_model_without_egnn_layers_is_plain():
    from pointvs_amd.screening import library_route, model_route
    assert library_route(None, False, False, False) == 'plain'
    assert model_route(SimpleNamespace(layers=[object()])) == 'plain'


def test_capture_refusal_gives_the_two_messages_and_none_otherwise():
    """The steps take the screen they serve; what capture_refusal reads of it needs no device."""
    from pointvs_amd.library_steps import STEPS

    def screen(**kw):
        return SimpleNamespace(**dict(dict(struck=False, contact_attention=None, graphnorm=False, _gn_padded=False), **kw))
    assert set(STEPS) == {'plain', 'reuse', 'cropped'}
    plain = STEPS['plain'](screen()).capture_refusal()
    assert plain == ('capture needs the first-layer reuse (no edge_residual, no softmax attention - or '
                     'softmax_reuse=True -, hidden size 32 or 64)')
    assert STEPS['plain'](screen(graphnorm=True, _gn_padded=False)).capture_refusal() == plain
    exact = STEPS['reuse'](screen(graphnorm=True)).capture_refusal()
    assert exact == ('a graphnorm model normalises over the batch\'s nodes and runs at the exact node '
                     'count: it cannot be captured at the padded shape; call the screen eagerly')
    assert STEPS['reuse'](screen()).capture_refusal() is None
    assert STEPS['reuse'](screen(graphnorm=True, _gn_padded=True)).capture_refusal() is None
    assert STEPS['reuse'](screen(struck=True, contact_attention=None)).capture_refusal() is None
    assert STEPS['cropped'](screen()).capture_refusal() is None
    assert STEPS['cropped'](screen(graphnorm=True, _gn_padded=True)).capture_refusal() is None
    assert [STEPS[r].has_builder for r in ('plain', 'reuse', 'cropped')] == [False, True, True]


def test_the_plain_step_refuses_what_it_cannot_do_in_the_present_words():
    from pointvs_amd.library_steps import STEPS
    with pytest.raises(ValueError, match='struck slots are built for the step of the first-layer reuse'):
        STEPS['plain'](SimpleNamespace(struck=True, contact_attention=None))
    with pytest.raises(NotImplementedError, match=r'LibraryScreen\(contact_attention=-1\): the contact-attention '
                                                  'reduction runs in the step of the first-layer reuse'):
        STEPS['plain'](SimpleNamespace(struck=False, contact_attention=2, _contact_request=-1))
