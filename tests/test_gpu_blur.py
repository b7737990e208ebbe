"""csrc/blur.hip on the GPU against the float64 reference on every case of tests/blur_reference.py (whose docstring
states the tolerance rule: 8 x the float32 evaluation's own error, floored at a few float32 ulps; counts equal), run to
run bit-identity, the workspace check, and the convention pin: the statistic agrees with the renderer it describes."""
import ctypes

import numpy as np
import pytest
import torch

import blur_reference as R

pytestmark = pytest.mark.gpu

CASES = R.cases()
IDS = [c["name"] for c in CASES]


def tensors(c, dev):
    return [torch.from_numpy(c[k]).to(dev) for k in ("points", "viewmats", "lin", "ang", "intrins", "times")]


def as_dict(stats):
    return {"count": stats.count.cpu().numpy(), **{k: getattr(stats, k).cpu().numpy() for k in R.STATS}}


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_against_the_reference(gs, dev, c):
    stats = gs.blur_stats(*tensors(c, dev), c["W"], c["H"])
    F = c["viewmats"].shape[0]
    assert stats.count.is_cuda and stats.count.dtype == torch.int32 and stats.count.shape == (F,)
    assert all(getattr(stats, k).dtype == torch.float32 and getattr(stats, k).shape == (F,) for k in R.STATS)
    got = as_dict(stats)
    R.check(c, got, "hip")
    if c["name"] == "zeros":                                  # exact zeros, not small numbers
        for f, zero in ((0, ("mean_blur", "rms_blur", "max_blur")), (1, ("mean_skew",)), (2, R.STATS), (3, R.STATS)):
            assert all(got[k][f] == 0.0 for k in zero), (f, got)
    if c["name"] == "looking_away":
        assert got["count"][3] == 0 and all(got[k][3] == 0.0 for k in R.STATS)


@pytest.mark.parametrize("ppt", [1, 2, 4, 8, 16])
def test_every_points_per_thread_variant(gs, dev, ppt):
    """the tuning knob reorders float64 sums and nothing else: every variant meets the same tolerance on the case with
    two frame groups and a chunk and one point"""
    c = next(c for c in CASES if c["name"] == "F33")
    R.check(c, as_dict(gs.blurscore.blur_stats_hip(*tensors(c, dev), c["W"], c["H"], points_per_thread=ppt)), f"hip ppt={ppt}")


def test_two_calls_are_bit_identical(gs, dev):
    for name in ("N3001", "F33"):
        c = next(c for c in CASES if c["name"] == name)
        t = tensors(c, dev)
        a = gs.blur_stats(*t, c["W"], c["H"])
        b = gs.blur_stats(*t, c["W"], c["H"])
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def test_empty_shapes_launch_nothing_and_return_zeros(gs, dev):
    c = CASES[1]
    t = tensors(c, dev)
    none = gs.blur_stats(t[0][:0], *t[1:], c["W"], c["H"])
    assert none.count.tolist() == [0] * 7 and all(float(getattr(none, k).abs().max()) == 0.0 for k in R.STATS)
    assert gs.blur_stats(t[0], *(x[:0] for x in t[1:]), c["W"], c["H"]).count.shape == (0,)


def test_small_workspace_is_refused(gs, dev):
    from gsdeblur_amd import _lib
    c = next(c for c in CASES if c["name"] == "N3001")
    t = tensors(c, dev)
    need = int(_lib.load().gs_blur_stats_workspace_bytes(7, 3001))
    assert need == 3 * 7 * 32
    with pytest.raises(_lib.HipLibraryError, match="workspace too small"):
        gs.blurscore.blur_stats_hip(*t, c["W"], c["H"], workspace_bytes=need - 1)
    R.check(c, as_dict(gs.blurscore.blur_stats_hip(*t, c["W"], c["H"], workspace_bytes=need)), "hip exact workspace")
    # the plain entry point, called directly: the same code
    lib, vp = _lib.load(), ctypes.c_void_p
    counts = torch.zeros(7, dtype=torch.int32, device=dev)
    stats = torch.zeros(7, 4, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    status = lib.gs_blur_stats(7, 3001, vp(t[0].data_ptr()), vp(t[1].data_ptr()), vp(t[2].data_ptr()), vp(t[3].data_ptr()),
                               vp(t[4].data_ptr()), vp(t[5].data_ptr()), c["W"], c["H"], 0.01, vp(counts.data_ptr()),
                               vp(stats.data_ptr()), vp(ws.data_ptr()), need - 1, None)
    assert status == 3
    torch.cuda.synchronize()
    assert int(counts.abs().max()) == 0                       # nothing ran


def test_convention_pin_against_the_renderer(gs, dev):
    """the first-order streak E |pv| of the statistic against what the renderer's own projection does over the exposure:
    the points projected with gs.project_gaussians under gs.subpose_viewmats at t = -E/2 and t = +E/2.  The reference's
    float64 gap between first order and the exact screw is below 1 % per frame (asserted in pin_case), the comparison is to
    5 %; a wrong axis flip, velocity frame or time origin misses by order one."""
    c, scale = R.pin_case()
    exact, first, sel = R.exact_displacement(c, 2.0)
    assert (np.abs(exact - first) < 0.01 * first).all()
    pts, V, lin, ang, intr, times = tensors(c, dev)
    for f in range(V.shape[0]):
        idx = torch.from_numpy(np.nonzero(sel[f])[0]).to(dev)
        p = pts[idx].contiguous()
        n = p.shape[0]
        E = float(times[f, 0])
        ends = gs.subpose_viewmats(V[f], lin[f], ang[f], torch.tensor([-0.5 * E, 0.5 * E], device=dev))
        fx, fy, cx, cy = (float(v) for v in intr[f])
        quats = torch.tensor([1.0, 0.0, 0.0, 0.0], device=dev).repeat(n, 1)
        xys = []
        for vm in ends:
            out = gs.project_gaussians(p, torch.full((n, 3), 1e-3, device=dev), 1.0, quats, vm.contiguous(), fx, fy, cx, cy,
                                       c["H"], c["W"])
            assert bool((out[2] > 0).all())                    # every selected point is on screen at both ends
            xys.append(out[0].double())
        moved = float((xys[1] - xys[0]).norm(dim=1).mean())
        stats = gs.blur_stats(p, V[f:f + 1], lin[f:f + 1], ang[f:f + 1], intr[f:f + 1], times[f:f + 1], c["W"], c["H"])
        assert int(stats.count[0]) == n
        mean_blur = float(stats.mean_blur[0])
        print(f"frame {f}: renderer moves {moved:.5f} px, mean_blur {mean_blur:.5f} px, float64 exact {exact[f]:.5f}")
        assert abs(moved - mean_blur) < 0.05 * mean_blur, (f, moved, mean_blur)
        assert abs(mean_blur - first[f]) < 1e-4 * first[f]
