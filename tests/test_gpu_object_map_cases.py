"""-m gpu: the life cycles of tests/object_map_cases.py on the device.  Every case runs three ways (object_map_cases.run_three): the
reused context with khr_integrate_shared_batch, a fresh context frame by frame, a fresh OracleMap.  Batch against frame by frame is
bit for bit in both arithmetic modes; the device against the oracle is common.compare_maps and common.TOL for the mesh points.
tests/test_cpu_object_map_cases.py shows on the oracle alone that every case is what it claims to be.

Two defects showed here first.  Before k_multi_order strode over all items, M1, M2 and M3 failed in both arithmetic modes with a digest
mismatch between the batch and the frame-by-frame context in every value layer (blocks beyond the slots its grid covered received
no frame of the batch).  Before khr_reset_map cleared the update kernels' per-workgroup statistics, R1 to R6 failed on
cum_updated_voxels alone (R1: 780982 against 36091): the last call before the reset was counted once more after it; their maps,
prune counts and meshes were equal.  The C and B cases passed before either change."""
import pytest

import object_map_cases as oc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("exact", [1, 0])
@pytest.mark.parametrize("name", oc.R_CASES)
def test_reused_context_equals_a_fresh_one(name, exact):
    """group R: the later object of a context that was reset to another voxel size, against a context that saw only that object"""
    oc.run_three(oc.CASES[name], exact=exact)


@pytest.mark.parametrize("exact", [1, 0])
@pytest.mark.parametrize("name", oc.M_CASES)
def test_batch_reaches_blocks_of_an_allocating_frame_or_a_checkpoint(name, exact):
    """group M: more updated blocks than the explicitly allocated ones account for in the launch of k_multi_order"""
    oc.run_three(oc.CASES[name], exact=exact, max_oracle_blocks=120)


@pytest.mark.parametrize("name", oc.C_CASES)
def test_cull_branches(name):
    """group C: the extractor's configuration in exact arithmetic, one branch of k_multi_cull per case"""
    oc.run_three(oc.CASES[name], exact=1)


@pytest.mark.parametrize("layout,exact", [("object", 0), ("label", 1), ("label", 0)])
@pytest.mark.parametrize("name", oc.C_AGAIN)
def test_cull_branches_relaxed_and_label_map(name, layout, exact):
    """camera inside the box, general camera, partial last tiles: in relaxed arithmetic and through k_fuse2<8, 4, ..> as well"""
    oc.run_three(oc.variant(name, layout), exact=exact)


@pytest.mark.parametrize("exact", [1, 0])
def test_band_rows_on_the_batch_path(exact):
    """group B: 20 labels in padded rows and a mini context for frames above 640 x 480 -- fuseBandRows<8, CAP> inside k_fuse2's
    multi-frame form, three launches -- and the same case in a 320 x 240 context (fuseBandRecord): one digest"""
    rows = oc.run_three(oc.CASES["B_rows"], exact=exact)
    records = oc.run_three(oc.CASES["B_records"], exact=exact)
    assert rows == records
