"""Host side of per-instance contact placements, no GPU: the tables robotoc_amd.solver builds from a ContactPlan (shared, per
instance, mixed), and the library's new entry points as the Python binding sees them."""
import numpy as np
import pytest

from robotoc_amd import capi
from robotoc_amd.grid import ContactSequence, Event, discretize
from robotoc_amd.solver import ContactPlan, placement_tables
from robotoc_amd.types import GRID_IMPACT, GRID_LIFT


def _grids():
    return discretize(6, 0.12, 0.0, ContactSequence([12, 6, 12], [Event("lift", 0.03), Event("impact", 0.07, impact_dimf=6)]))


def _phase_of(grids):
    out, p = [], 0
    for g in grids:
        if g.type in (GRID_IMPACT, GRID_LIFT):
            p += 1
        out.append(p)
    return out


def test_a_plan_of_the_old_shape_gives_the_shared_tables_as_before():
    grids, rng = _grids(), np.random.default_rng(0)
    pp = [rng.uniform(-1, 1, (4, 3)) for _ in range(3)]
    pr_ = [rng.uniform(-1, 1, (4, 3, 3)) for _ in range(3)]
    pos, rot, inst = placement_tables(ContactPlan([15, 9, 15], pp, phase_rotations=pr_), grids, 4, 5)
    assert inst is False and pos.shape == (len(grids), 4, 3) and rot.shape == (len(grids), 4, 3, 3)
    for i, p in enumerate(_phase_of(grids)):
        assert np.array_equal(pos[i], pp[p]) and np.array_equal(rot[i], pr_[p])
    pos, rot, inst = placement_tables(ContactPlan([15, 9, 15], [x.tolist() for x in pp]), grids, 4, 5)   # lists, no rotations
    assert inst is False and rot is None and np.array_equal(pos[-1], pp[2])
    # fewer phases given than the grid has: the last one holds (as before)
    pos, _, _ = placement_tables(ContactPlan([15, 9, 15], pp[:1]), grids, 4, 5)
    assert all(np.array_equal(pos[i], pp[0]) for i in range(len(grids)))


def test_a_per_instance_plan_gives_tables_with_a_leading_batch():
    grids, rng, batch = _grids(), np.random.default_rng(1), 3
    pp = [rng.uniform(-1, 1, (batch, 4, 3)) for _ in range(3)]
    pr_ = [rng.uniform(-1, 1, (batch, 4, 3, 3)) for _ in range(3)]
    pos, rot, inst = placement_tables(ContactPlan([15, 9, 15], pp, phase_rotations=pr_), grids, 4, batch)
    assert inst is True and pos.shape == (batch, len(grids), 4, 3) and rot.shape == (batch, len(grids), 4, 3, 3)
    assert pos.flags["C_CONTIGUOUS"] and rot.flags["C_CONTIGUOUS"]
    for i, p in enumerate(_phase_of(grids)):
        for b in range(batch):
            assert np.array_equal(pos[b, i], pp[p][b]) and np.array_equal(rot[b, i], pr_[p][b])


def test_a_plan_that_mixes_the_two_shapes_is_refused():
    grids, batch = _grids(), 3
    with pytest.raises(ValueError):
        placement_tables(ContactPlan([15, 9, 15], [np.zeros((4, 3)), np.zeros((batch, 4, 3)), np.zeros((4, 3))]), grids, 4, batch)
    with pytest.raises(ValueError):   # positions per instance, rotations shared
        placement_tables(ContactPlan([15, 9, 15], [np.zeros((batch, 4, 3))] * 3, phase_rotations=[np.zeros((4, 3, 3))] * 3), grids, 4, batch)
    with pytest.raises(ValueError):   # neither shape
        placement_tables(ContactPlan([15, 9, 15], [np.zeros((2, 4, 3))] * 3), grids, 4, batch)


def test_the_library_exports_the_placement_entry_points():
    L = capi.lib()
    for name in ("rtoc_set_contact_placements", "rtoc_contact_frame_placements", "rtoc_hold_contact_placements", "rtoc_get_contact_placements"):
        assert name in capi.EXPORTS and hasattr(L, name)
    # a null context is refused ahead of everything else
    assert L.rtoc_set_contact_placements(None, None, None, 1) == -1
    assert L.rtoc_hold_contact_placements(None, 0, 0, 0, 1, 1) == -1
    assert L.rtoc_contact_frame_placements(None, 0, 0, None, None, None, 0) == -1
