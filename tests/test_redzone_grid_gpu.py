"""The lattice, bit-grid and compaction kernels (csrc/grid_common.hpp: two-word ballot stores, count / prefix / write compactions) inside
tests/redzone.py: k_occupancy_bits, the cull, the carve counters / bits / lattice, the cloud sums / points / labels.  Every row twice, fill 0x00 then
0xFF, inputs placed flush against guards, outputs, scratch words and block counts carved: no guard byte and no input changed, the results equal bit
for bit.  The compaction outputs are allocated at the kept count M, so they have no don't-care tail.  carve_accumulate and cloud_accumulate update
``counts`` / ``sums`` in place, as their docstrings say; those placed tensors are named as written and are the rows' results.  Bytes are held to
the restatements by tests/test_skip_empty_gpu.py, tests/test_carve_gpu.py and tests/test_cloud_gpu.py, whose inputs are imported here; every kernel
here is integer or one fixed-order sum per element ("the same bytes on every call")."""
import numpy as np
import pytest
import torch

import carve_ref as CR
import cloud_ref as CL
import skip_empty_ref as R
import test_cloud_gpu as TC
import test_skip_empty_gpu as TS
from redzone import both_fills

pytestmark = pytest.mark.gpu


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize("dilate", [0, 1, 2])
@pytest.mark.parametrize("nv", [(5, 3, 7), (8, 8, 40)])
def test_redzone_occupancy_bits(device, nv, dilate):
    """105 voxels: a ragged last word that a two-word ballot store must not spill past; (8, 8, 40): Z crosses a word boundary."""
    from nerfdet_amd import ops
    alpha, count, thr = TS._grid(nv)

    def body(rz):
        return {"bits": ops.occupancy_bits(rz.place(_t(alpha), "alpha"), rz.place(_t(count), "count"), nv, float(thr), dilate)}
    got = both_fills(device, body)
    assert np.array_equal(got["bits"].numpy(), R.occupancy_bits(alpha, count, nv, thr, dilate))


@pytest.mark.parametrize("n", [1, 65, 1025])
@pytest.mark.parametrize("outside", ["keep", "cull"])
@pytest.mark.parametrize("path", ["lds_odd", "global"])
def test_redzone_cull(device, path, outside, n):
    from nerfdet_amd import rays
    nv, p0, vs = TS.LATTICES[path]
    alpha, count, thr = TS._grid(nv)
    bits = R.occupancy_bits(alpha, count, nv, thr, 1)
    pts = TS._points(nv, p0, vs, n, seed=n)

    def body(rz):
        occ = rays.OccupancyGrid(rz.place(_t(bits), "bits"), nv, p0, vs, outside)
        idx, kept = rays.cull_points(rz.place(_t(pts), "pts"), occ)
        return {"idx": idx, "kept": kept}
    got = both_fills(device, body)
    want_idx, _ = R.cull(pts, bits, nv, p0, vs, outside)
    assert got["idx"].shape[0] == len(want_idx)


# ---- carve: counters, bits and lattice at (5, 3, 7), refine 4, k = 65 ----
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_redzone_carve_counters(device, dtype):
    from nerfdet_amd import ops
    nv, refine, k = (5, 3, 7), 4, 65
    pts = CR.fine_points(nv, refine)
    proj, depth = CR.views_case(nv, k, dtype)
    fine, vs_fine = ops.carve_lattice(nv, CR.VS, refine)
    assert fine == (20, 12, 28)
    n = fine[0] * fine[1] * fine[2]

    def body(rz):
        lattice = ops.get_points(fine, list(vs_fine), CR.ORIGIN, device)
        d = rz.place(_t(depth), "depth")
        counts = rz.place(torch.zeros(n, dtype=torch.int32), "counts")
        out = ops.carve_accumulate(counts, rz.place(pts, "points"), rz.place(proj, "projection"), ops.DepthGate(d, d, CR.BAND))
        assert out is counts
        return {"counts": counts, "lattice": lattice}
    got = both_fills(device, body, written=("counts",))          # carve_accumulate: "In place ...; returns ``counts``"
    assert torch.equal(got["lattice"], pts)


@pytest.mark.parametrize("two_pass", [False, True])
@pytest.mark.parametrize("dilate,with_coarse", [(0, False), (1, True), (2, True)])
@pytest.mark.parametrize("n_segs", [1, 64])
def test_redzone_carve_bits(device, n_segs, dilate, with_coarse, two_pass):
    """(5, 3, 7) as the fine lattice itself (105 voxels: a ragged last word) and refined 4 times from it (20, 12, 28) with the coarse grid's bits."""
    from nerfdet_amd import ops
    for nv, r in (((5, 3, 7), 1), ((20, 12, 28), 4)):
        n = nv[0] * nv[1] * nv[2]
        segs = CR.segments_case(n, n_segs, seed=n_segs)
        coarse = R.pack_bits(np.random.RandomState(9).rand(n // r ** 3) < 0.7)

        def body(rz):
            dev = [rz.place(_t(s), f"segment{i}") for i, s in enumerate(segs)]
            cb = rz.place(_t(coarse), "coarse_bits") if with_coarse else None
            return {"bits": ops.carve_bits(dev, nv, 2, dilate, cb, r, two_pass=two_pass)}
        got = both_fills(device, body)
        assert np.array_equal(got["bits"].numpy(), CR.bits(segs, nv, 2, dilate, coarse if with_coarse else None, r))


# ---- cloud ----
@pytest.mark.parametrize("merge", [True, False])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_redzone_cloud_sums(device, dtype, merge):
    """The odd frame size of tests/test_cloud_gpu.py (views straddle waves, the last wave is partial) on the standard lattice refined twice."""
    from nerfdet_amd import ops
    case = CL.standard_case(dtype, hw=CL.ODD_HW)
    nv, p0, vs = TC._lattice(2)
    n = nv[0] * nv[1] * nv[2]

    def body(rz):
        sums = rz.place(torch.zeros(n, ops.CLOUD_WORDS, dtype=torch.int32), "sums")
        out = ops.cloud_accumulate(sums, nv, p0, vs, rz.place(_t(case["depth"]), "depth"), rz.place(_t(case["rgb"]), "rgb"), case["intrinsic"],
                                   case["c2w"], None, merge=merge)
        assert out is sums
        return {"sums": sums}
    got = both_fills(device, body, written=("sums",))            # cloud_accumulate: "In place ...; returns ``sums``"
    assert bool(got["sums"].any())


@pytest.mark.parametrize("n_segs,min_points", [(1, 1), (2, 3), (64, 1)])
def test_redzone_cloud_points_and_labels(device, n_segs, min_points):
    """(7, 9, 41): 2583 voxels, a partial workgroup and a partial 512-voxel block; then k_label_points over the emitted points."""
    from nerfdet_amd import ops, pipeline
    from nerfdet_amd.boxes import box_frames
    nv = (7, 9, 41)
    n = nv[0] * nv[1] * nv[2]
    p0, vs = np.float32([-0.4, 1.3, 0.05]), np.float32([0.1, 0.07, 0.3])
    segs, _ = TC._record_segments(n, n_segs, seed=n_segs)
    bf = box_frames(CL.boxes7())

    def body(rz):
        dev = [rz.place(_t(s), f"segment{i}") for i, s in enumerate(segs)]
        out = ops.cloud_points(dev, nv, p0, vs, min_points)
        out["labels"] = pipeline.label_points(out["xyz"], bf)
        return out
    got = both_fills(device, body)
    assert got["voxel"].numel() > 0 and got["labels"].shape == got["voxel"].shape
