"""Alias of /root/reference/point_vs/attribution/attribution_fns.py (atom_masking :356-456, bond_masking :39-115,
cam :298-353, node_attention :238-275, edge_attention :278-295) -> pointvs_amd.attribution.

`SIGMOID` is a module-level switch there and here. The functions read it from this module at call time, so
`attribution_fns.SIGMOID = True` works as it does against the reference."""
import functools
import sys

from pointvs_amd import attribution as _impl

SIGMOID = False


def _follow_switch(fn):
    @functools.wraps(fn)
    def call(*args, **kwargs):
        _impl.SIGMOID = bool(sys.modules[__name__].SIGMOID)
        return fn(*args, **kwargs)
    return call


atom_masking = _follow_switch(_impl.atom_masking)
bond_masking = _follow_switch(_impl.bond_masking)
cam = _follow_switch(_impl.cam)
node_attention = _follow_switch(_impl.node_attention)
edge_attention = _follow_switch(_impl.edge_attention)
