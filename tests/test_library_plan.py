"""plan_library: the host-side batch plan of a library sweep (pointvs_amd/screening.py). No GPU."""
import pytest


def _check(plan, pose_counts, batch_size):
    want = [(lig, pose) for lig, count in enumerate(pose_counts) for pose in range(count)]
    assert [pair for batch in plan for pair in batch] == want       # every (ligand, pose) once, in order
    assert len(plan) == -(-len(want) // batch_size)
    assert all(len(batch) == batch_size for batch in plan[:-1])      # dense: only the last batch may be short
    assert not plan or 1 <= len(plan[-1]) <= batch_size


def test_plan_fills_slots_densely_in_library_then_pose_order():
    from pointvs_amd.screening import plan_library
    counts, sizes = (7, 0, 5, 130), (12, 9, 64, 1)
    plan = plan_library(counts, sizes, 4, 64)
    _check(plan, counts, 4)
    assert len(plan) == 36 and len(plan[-1]) == 2
    assert plan[1] == [(0, 4), (0, 5), (0, 6), (2, 0)]               # a batch mixes ligands; ligand 1 has no pose


def test_plan_of_a_library_that_exactly_fills_its_last_batch():
    from pointvs_amd.screening import plan_library
    counts, sizes = (3, 9, 4), (8, 60, 33)
    plan = plan_library(counts, sizes, 8, 64)
    _check(plan, counts, 8)
    assert len(plan) == 2 and len(plan[-1]) == 8
    assert plan_library((), (), 8, 64) == []


def test_plan_rejects_a_ligand_above_the_slot_size():
    from pointvs_amd.screening import plan_library
    with pytest.raises(ValueError):
        plan_library((2, 3), (12, 65), 4, 64)
    with pytest.raises(ValueError):
        plan_library((2, 3), (12, 20), 4, 16)
    with pytest.raises(ValueError):
        plan_library((2,), (0,), 4, 64)
    assert plan_library((2, 0), (12, 65), 4, 64) == [[(0, 0), (0, 1)]]    # no pose, no slot: nothing to reject
