"""Alias of /root/reference/point_vs/attribution: the attribution functions of the geometric models
(`attribution_fns`) -> pointvs_amd.attribution. PDB parsing, PLIP, PyMOL and `attribute()` are out of scope."""
