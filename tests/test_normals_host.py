"""The depth-derived normals and their two losses on the CPU: csrc/normal_math.h compiled with g++ and normal_loss_torch
against the float64 reference (tests/normal_reference.py, whose docstring states the tolerance rule); the reference's
gradient against float64 autograd of a plain torch statement of the loss; known answers and the smallest frames; the
Python surface, the training surface with a stand-in render, the loaders, the C-ABI entries and the tools' flags."""
import ctypes
import re
import struct
import subprocess
import types
import zlib
from pathlib import Path

import numpy as np
import pytest
import torch

import normal_reference as R

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "host_math" / "normal_host.cpp"
LIB = ROOT / "tests" / "host_math" / "libnormal_host.so"
CSRC = ROOT / "3dgs-deblur_amd" / "csrc"
HDRS = (CSRC / "normal_math.h", CSRC / "depthprior_math.h")
HIP = CSRC / "normals.hip"
NEW_EXPORTS = {"gs_depth_normals": 10, "gs_normal_loss_workspace_bytes": 4, "gs_normal_loss": 21}


def kernel_constant(name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, HIP.read_text()).group(1))


TW, TH, GROUP, K_THREADS = (kernel_constant(k) for k in ("kTileW", "kTileH", "kGroupTiles", "kThreads"))
SMALL = [(1, 1), (2, 5), (5, 2), (3, 3), (3, 4), (4, 3), (7, 13), (67, 131)]                 # (H, W)
TILE_EDGES = [(TH + 1, w) for w in (TW - 1, TW, TW + 1, 2 * TW + 1)] + [(h, TW + 1) for h in (TH - 1, TH, TH + 1, 2 * TH + 1)]
GROUP_EDGE = [(TH + 1, GROUP * TW + 1)]            # a second workgroup in x
MANY_GROUPS = (TH * K_THREADS + 1, TW + 1)         # more records than the gradient kernel's workgroup has threads
SIZES = SMALL + TILE_EDGES + GROUP_EDGE


def P(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def nmh():
    if not LIB.exists() or LIB.stat().st_mtime < max(f.stat().st_mtime for f in (SRC,) + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", f"-I{CSRC}", str(SRC),
                               "-o", str(LIB)])
    lib = ctypes.CDLL(str(LIB))
    lib.nmh_min_l2.restype = ctypes.c_float
    lib.nmh_normal_loss.restype = None
    lib.nmh_normal_loss.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p] * 5 + [ctypes.c_float] * 4 + [ctypes.c_void_p] * 5
    return lib


def term_args(term, prior, guide):
    t = R.TERMS[term]
    kw = dict(prior_weight=t["prior_weight"], smooth_weight=t["smooth_weight"], edge_beta=t["edge_beta"])
    return (prior if t["use_prior"] else None), (guide if t["use_guide"] else None), kw


def host_loss(lib, acc, al, K, prior=None, guide=None, prior_weight=1.0, smooth_weight=0.0, edge_beta=0.0, min_alpha=0.0):
    """the host-compiled header on [B,S,H,W] arrays -> loss [B], v_depth_acc, v_alphas, stats [B,6], normals [B,H,W,3]"""
    acc, al, K = (np.ascontiguousarray(t, np.float32) for t in (acc, al, K))
    prior = None if prior is None else np.ascontiguousarray(prior, np.float32)
    guide = None if guide is None else np.ascontiguousarray(guide, np.float32)
    B, S, H, W = acc.shape
    loss, stats, n = np.empty(B, np.float32), np.empty((B, 6), np.float64), np.empty((B, H, W, 3), np.float32)
    vd, va = np.empty_like(acc), np.empty_like(al)
    lib.nmh_normal_loss(B, S, H, W, P(acc), P(al), P(K), P(prior), P(guide), prior_weight, smooth_weight, edge_beta, min_alpha,
                        P(loss), P(stats), P(n), P(vd), P(va))
    return loss, vd, va, stats, n


def torch_loss(gs, acc, al, K, prior=None, guide=None, **kw):
    f = lambda t: None if t is None else torch.from_numpy(np.ascontiguousarray(t, np.float32))   # noqa: E731
    out = gs.normals.normal_loss_torch(f(acc), f(al), f(K), f(prior), f(guide), return_stats=True, return_normals=True, **kw)
    return tuple(t.numpy() for t in out)


# --------------------------------------------------------------------------- #
# the op against the reference
# --------------------------------------------------------------------------- #
def test_constants_agree(gs, nmh):
    assert nmh.nmh_stats() == gs.normals.STATS == 6
    assert nmh.nmh_min_l2() == np.float32(gs.normals.MIN_L2) == R.MIN_L2
    assert TW * TH == K_THREADS and GROUP >= 1


def test_sizes_cover_what_they_claim():
    assert {(1, 1), (2, 5), (5, 2), (3, 3), (3, 4), (4, 3), (7, 13), (67, 131)} <= set(SIZES)
    assert {w for h, w in SIZES if h == TH + 1} >= {TW - 1, TW, TW + 1, 2 * TW + 1, GROUP * TW + 1}
    assert {h for h, w in SIZES if w == TW + 1} >= {TH - 1, TH, TH + 1, 2 * TH + 1}
    groups = -(-MANY_GROUPS[1] // (TW * GROUP)) * -(-MANY_GROUPS[0] // TH)
    assert groups > K_THREADS                                   # the record loop takes a second trip


# the large size at S = 1, B = 1 only here; the GPU tests run every combination
HOST_CASES = [(size, S, B) for size in SIZES for S, B in ((1, 1), (5, 3))] + [(MANY_GROUPS, 1, 1)]


@pytest.mark.parametrize("size,S,B", HOST_CASES, ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v))
def test_header_and_torch_restatement_match_the_reference(gs, nmh, size, S, B):
    H, W = size
    acc, al, K, prior, guide = R.make_batch(B, S, H, W, seed=11 + H + W)
    for b in range(B):
        R.assert_input_conditions(acc[b], al[b], K[b], prior[b])
    for term in R.TERMS:
        pr, gd, kw = term_args(term, prior, guide)
        for name, got in (("header", host_loss(nmh, acc, al, K, pr, gd, **kw)), ("torch", torch_loss(gs, acc, al, K, pr, gd, **kw))):
            for b in range(B):
                fig = R.check_frame(got[0][b], got[1][b], got[2][b], got[4][b], got[3][b], acc[b], al[b], K[b],
                                    what=(name, term, S, b, size), prior=None if pr is None else pr[b],
                                    guide=None if gd is None else gd[b], **kw)
                if b == 0 and H >= 4 and W >= 4:
                    assert got[1][b].any() and got[2][b].any(), (name, term, size)
        print(term, fig)
    if B == 3:                                  # alpha 0 everywhere: nothing at all; no prior value: no prior term
        ref = R.reference(acc[1], al[1], K[1], prior=prior[1])
        assert ref["stats"][1] == 0 and (ref["stats"][0] > 0 or H < 3 or W < 3)
        assert R.reference(acc[2], al[2], K[2], prior=prior[2])["stats"][0] == 0


def plain_loss(acc, al, K, prior, guide, defined, use, prior_weight, smooth_weight, edge_beta):
    """the loss as a plain float64 torch statement with the reference's masks (constants): slices, torch.cross, mean"""
    S, H, W = acc.shape
    z = (acc.sum(0) / S) / torch.where(al.sum(0) > 0, al.sum(0) / S, torch.ones((), dtype=torch.float64))
    fx, fy, cx, cy = (float(np.float32(k)) for k in K)
    u, v = torch.arange(W, dtype=torch.float64), torch.arange(H, dtype=torch.float64)
    Pt = torch.stack([((u + 0.5 - cx) / fx)[None, :] * z, ((v + 0.5 - cy) / fy)[:, None] * z, z], -1)
    c = torch.linalg.cross(Pt[2:, 1:-1] - Pt[:-2, 1:-1], Pt[1:-1, 2:] - Pt[1:-1, :-2])
    inner = torch.from_numpy(defined[1:-1, 1:-1])
    one, zero = torch.ones((), dtype=torch.float64), torch.zeros((), dtype=torch.float64)
    length = torch.sqrt(torch.where(inner, (c * c).sum(-1), one))          # (no square root of 0 on the tape)
    n = torch.zeros(H, W, 3, dtype=torch.float64)
    n[1:-1, 1:-1] = torch.where(inner[..., None], c / length[..., None], zero)
    loss = torch.zeros((), dtype=torch.float64)
    if prior is not None and use.any():
        m = torch.from_numpy(prior).double()
        m = m / torch.where(torch.from_numpy(use), m.norm(dim=-1), torch.ones(()).double())[..., None]
        loss = loss + prior_weight * (1.0 - (n * m).sum(-1))[torch.from_numpy(use)].mean()
    terms = []
    dfn = torch.from_numpy(defined)
    gd = None if guide is None or not edge_beta > 0 else torch.from_numpy(guide).double()
    for a, b in (((slice(None), slice(0, -1)), (slice(None), slice(1, None))), ((slice(0, -1), slice(None)), (slice(1, None), slice(None)))):
        both = dfn[a] & dfn[b]
        g = torch.ones(both.shape, dtype=torch.float64) if gd is None else torch.exp(-edge_beta * (gd[a] - gd[b]).abs().mean(-1))
        terms.append((g * (1.0 - (n[a] * n[b]).sum(-1)))[both])
    terms = torch.cat(terms)
    if terms.numel():
        loss = loss + smooth_weight * terms.mean()
    return loss


@pytest.mark.parametrize("size", [(9, 11), (67, 131)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("S", [1, 5])
def test_reference_gradient_is_float64_autograd_of_plain_torch(size, S):
    """reference(store=None) is all float64, and so is autograd of the plain statement on the same numbers: they differ by
    float64 rounding alone (1e-9 relative leaves six digits of room)"""
    H, W = size
    acc, al, K, prior, guide = R.make_frame(S, H, W, seed=5)
    for term in R.TERMS:
        pr, gd, kw = term_args(term, prior, guide)
        # float32 weights, as the C ABI takes them; the guide's float64 exp has no float32 step at store=None
        w = {k: float(np.float32(v)) for k, v in kw.items()}
        ref = R.reference(acc, al, K, prior=pr, guide=gd, store=None, **kw)
        a64 = torch.from_numpy(acc).double().requires_grad_(True)
        l64 = torch.from_numpy(al).double().requires_grad_(True)
        use = ref["defined"] & ((pr.astype(np.float64) ** 2).sum(-1) > 0) if pr is not None else np.zeros((H, W), bool)
        loss = plain_loss(a64, l64, K, pr, gd, ref["defined"], use, w["prior_weight"], w["smooth_weight"], w["edge_beta"])
        loss.backward()
        assert abs(float(loss.detach()) - ref["loss"]) < 1e-12
        for got, want in ((ref["v_depth_acc"], a64.grad.numpy()), (ref["v_alphas"], l64.grad.numpy())):
            assert np.abs(want).max() > 0
            assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), term


# --------------------------------------------------------------------------- #
# known answers and the smallest frames
# --------------------------------------------------------------------------- #
def _plane(H, W, a=0.0, b=0.0, z0=4.0):
    """one sample, alpha 1, the plane z (1 - a rx - b ry) = z0, i.e. the points with (a, b, 1) . P = z0"""
    K = R.intrinsics(H, W)
    u, v = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    rx, ry = ((u + 0.5 - K[2]) / K[0])[None, :], ((v + 0.5 - K[3]) / K[1])[:, None]
    z = z0 / (1.0 + a * rx + b * ry)
    return z[None].astype(np.float32), np.ones((1, H, W), np.float32), K


def both(gs, nmh, acc, al, K, **kw):
    """(loss, v_depth_acc, v_alphas, stats, normals) of one frame from the host-compiled header and the torch restatement"""
    pr, gd = kw.pop("prior", None), kw.pop("guide", None)
    h = host_loss(nmh, acc[None], al[None], K[None], None if pr is None else pr[None], None if gd is None else gd[None], **kw)
    t = torch_loss(gs, acc, al, K, pr, gd, **kw)
    return tuple(x[0] for x in h), t


def test_a_fronto_parallel_plane_is_exact(gs, nmh):
    acc, al, K = _plane(23, 31)
    for loss, vd, va, stats, n in both(gs, nmh, acc, al, K, prior_weight=0.0, smooth_weight=0.4):
        assert stats[0] == 21 * 29 and stats[3] == 21 * 28 + 20 * 29
        assert np.array_equal(n[1:-1, 1:-1], np.broadcast_to(np.float32([0, 0, -1]), (21, 29, 3))) and not n[0].any()
        assert stats[4] == 0.0 and float(loss) == 0.0 and not vd.any() and not va.any()


def test_a_tilted_plane_has_its_own_normal(gs, nmh):
    a, b = 0.3, -0.2
    acc, al, K = _plane(23, 31, a, b)
    want = -np.array([a, b, 1.0]) / np.sqrt(a * a + b * b + 1.0)
    _, _, tol = R.tolerances(acc, al, K)
    for _, _, _, stats, n in both(gs, nmh, acc, al, K):
        assert stats[0] == 21 * 29
        assert np.abs(n[1:-1, 1:-1] - want).max() <= tol["normals"], (np.abs(n[1:-1, 1:-1] - want).max(), tol["normals"])
        assert ((n[1:-1, 1:-1] * want).sum(-1) > 0.999999).all()


def test_scaling_the_depth_by_four_changes_no_bit_of_the_normals(gs, nmh):
    acc, al, K, prior, guide = R.make_frame(5, 67, 131, seed=21)
    for one, four in zip(both(gs, nmh, acc, al, K, prior=prior), both(gs, nmh, (acc * 4).astype(np.float32), al, K, prior=prior)):
        assert np.array_equal(one[4], four[4]) and one[4].any() and float(one[0]) == float(four[0])


def test_normals_face_the_camera():
    acc, al, K, _, _ = R.make_frame(1, 67, 131, seed=8)
    r = R.reference(acc, al, K)
    z = acc[0] / np.where(al[0] > 0, al[0], 1)
    u, v = np.arange(131) + 0.5, np.arange(67) + 0.5
    Pt = np.stack([((u - K[2]) / K[0])[None, :] * z, ((v - K[3]) / K[1])[:, None] * z, z], -1)
    assert r["defined"].sum() > 1000 and ((r["normals"] * Pt).sum(-1)[r["defined"]] < 0).all()


@pytest.mark.parametrize("size,normals,pairs", [((1, 1), 0, 0), ((2, 5), 0, 0), ((5, 2), 0, 0), ((3, 3), 1, 0), ((3, 4), 2, 1),
                                                ((4, 3), 2, 1)], ids=str)
def test_the_smallest_frames(gs, nmh, size, normals, pairs):
    H, W = size
    acc, al, K, prior, guide = R.make_frame(2, H, W, seed=4)
    prior[...] = np.float32([0.1, 0.2, -1.0])
    for loss, vd, va, stats, n in both(gs, nmh, acc, al, K, prior=prior, guide=guide, prior_weight=0.7, smooth_weight=0.4,
                                       edge_beta=2.0):
        assert stats[0] == normals and stats[1] == normals and stats[3] == pairs
        assert (n != 0).any(-1).sum() == normals
        if normals == 0:
            assert float(loss) == 0.0 and not vd.any() and not va.any() and not n.any()
        else:
            assert float(loss) > 0 and vd.any() and va.any()
            # the centre of a single normal is not one of its four neighbours: it receives nothing
            assert normals > 1 or (not vd[:, 1, 1].any() and np.count_nonzero(vd[0]) == 4)


def test_a_pixel_without_z_gets_zeros_and_removes_five_normals(gs, nmh):
    acc, al, K, prior, guide = R.make_frame(3, 7, 9, seed=6)                   # (below 64 pixels: a frame without holes)
    full = both(gs, nmh, acc, al, K, prior=prior, smooth_weight=0.4)
    assert full[0][3][0] == 5 * 7
    al2, acc2 = al.copy(), acc.copy()
    al2[:, 3, 4] *= 0.01                                  # below min_alpha = 0.02: no z, although alpha and d are not 0
    for (loss, vd, va, stats, n), (_, _, _, stats0, n0) in zip(both(gs, nmh, acc2, al2, K, prior=prior, smooth_weight=0.4,
                                                                     min_alpha=0.02), full):
        gone = (n0 != 0).any(-1) & ~(n != 0).any(-1)
        want = np.zeros((7, 9), bool)
        want[3, 3:6] = want[2:5, 4] = True
        assert np.array_equal(gone, want) and stats[0] == stats0[0] - 5
        assert not vd[:, 3, 4].any() and not va[:, 3, 4].any() and vd[:, 3, 6].any()
        R.check_frame(loss, vd, va, n, stats, acc2, al2, K, prior=prior, smooth_weight=0.4, min_alpha=0.02)


# --------------------------------------------------------------------------- #
# the Python surface
# --------------------------------------------------------------------------- #
def test_argument_checks(gs):
    N = gs.normals
    acc, al, K = torch.rand(2, 4, 5) + 1, torch.rand(2, 4, 5) + 0.1, (4.0, 4.0, 2.5, 2.0)
    prior = torch.rand(4, 5, 3)
    for fn in (gs.normal_loss, gs.normal_loss_with_grad, N.normal_loss_torch):
        with pytest.raises(ValueError, match="float32"):
            fn(acc.double(), al, K)
        with pytest.raises(ValueError, match="alphas must have"):
            fn(acc, al[:1], K)
        with pytest.raises(ValueError, match="prior must be"):
            fn(acc, al, K, prior[None])
        with pytest.raises(ValueError, match="guide must be"):
            fn(acc, al, K, None, prior[:, :, :2])
        with pytest.raises(ValueError, match="intrins"):
            fn(acc, al, (4.0, 4.0, 2.5))
        with pytest.raises(ValueError, match="intrins"):
            fn(acc, al, (0.0, 4.0, 2.5, 2.0))
        with pytest.raises(ValueError, match="prior_weight"):
            fn(acc, al, K, prior, prior_weight=-1.0)
        with pytest.raises(ValueError, match="smooth_weight"):
            fn(acc, al, K, smooth_weight=float("nan"))
        with pytest.raises(ValueError, match="edge_beta"):
            fn(acc, al, K, edge_beta=-0.5)
        with pytest.raises(ValueError, match="min_alpha"):
            fn(acc, al, K, min_alpha=-0.1)
        with pytest.raises(ValueError, match="B \\* S"):
            fn(torch.rand(2, 129, 1, 1), torch.rand(2, 129, 1, 1), K)
    for fn in (gs.depth_normals, N.depth_normals_torch):
        with pytest.raises(ValueError, match="min_alpha"):
            fn(acc, al, K, -1.0)
        with pytest.raises(ValueError):
            fn(acc[0], al[0], K)
        assert fn(acc, al, K).shape == (4, 5, 3) and fn(acc[None].expand(3, 2, 4, 5), al[None].expand(3, 2, 4, 5), K).shape == (3, 4, 5, 3)
    with pytest.raises(ValueError, match="HIP"):
        N.normal_loss_hip(acc[None], al[None], K)
    with pytest.raises(ValueError, match="HIP"):
        N.depth_normals_hip(acc[None], al[None], K)
    assert gs.normal_loss is N.normal_loss and gs.depth_normals is N.depth_normals


def test_autograd_function_on_the_cpu(gs):
    acc, al, K, prior, guide = (torch.from_numpy(t) for t in R.make_batch(2, 3, 9, 11, seed=2))
    kw = dict(prior_weight=0.7, smooth_weight=0.4, edge_beta=2.0)
    loss, vd, va, stats, n = gs.normal_loss_with_grad(acc, al, K, prior, guide, return_stats=True, return_normals=True, **kw)
    assert loss.shape == (2,) and vd.shape == acc.shape and stats.shape == (2, 6) and n.shape == (2, 9, 11, 3)
    assert torch.equal(n, gs.depth_normals(acc, al, K))
    a, b = acc.clone().requires_grad_(True), al.clone().requires_grad_(True)
    out = gs.normal_loss(a, b, K, prior, guide, **kw)
    assert torch.equal(out.detach(), loss)
    (out * torch.tensor([1.0, 0.5])).sum().backward()
    assert torch.equal(a.grad[0], vd[0]) and torch.equal(a.grad[1], vd[1] * 0.5)
    assert torch.equal(b.grad[0], va[0]) and torch.equal(b.grad[1], va[1] * 0.5)
    # a single frame: a scalar, and the frame of a batch alone gives the batch's bits
    l0, vd0, va0 = gs.normal_loss_with_grad(acc[1], al[1], K[1], prior[1], guide[1], **kw)
    assert l0.shape == () and torch.equal(l0, loss[1]) and torch.equal(vd0, vd[1]) and torch.equal(va0, va[1])


# --------------------------------------------------------------------------- #
# the training surface, with a stand-in render on the CPU
# --------------------------------------------------------------------------- #
def _trainable(gs):
    from test_depthprior_host import TH as H, TW as W, _cpu_trainable
    model, cam, _, base, hole = _cpu_trainable(gs)
    g = torch.Generator().manual_seed(17)
    prior = torch.nn.functional.normalize(torch.randn(H, W, 3, generator=g) * 0.3 + torch.tensor([0.0, 0.0, -1.0]), dim=-1)
    prior[:, 3] = 0.0
    return model, cam, prior, base, hole, H, W


def test_train_step_rejects_bad_values_before_anything_runs(gs):
    T = gs.training
    model, cam, prior, _, _, H, W = _trainable(gs)
    model.get_outputs = lambda *a, **k: pytest.fail("rendered before the values were checked")
    opts = T.make_optimizers(model)
    img = torch.full((H, W, 3), 0.5)
    with pytest.raises(ValueError, match="normal_lambda"):
        T.train_step(model, opts, cam, img, gt_normal=prior, normal_lambda=-0.1)
    with pytest.raises(ValueError, match="normal_smooth_lambda"):
        T.train_step(model, opts, cam, img, normal_smooth_lambda=float("nan"))
    with pytest.raises(ValueError, match="normal_edge_beta"):
        T.train_step(model, opts, cam, img, normal_smooth_lambda=0.1, normal_edge_beta=-1.0)
    with pytest.raises(ValueError, match="gt_normal"):
        T.train_step(model, opts, cam, img, gt_normal=prior[..., :1], normal_lambda=0.1)
    with pytest.raises(ValueError, match="gt_normal"):
        T.train_step(model, opts, [cam], [img], gt_normal=[prior[0]], normal_lambda=0.1)
    scene = types.SimpleNamespace(cameras=[cam], train_indices=[0], eval_indices=[0])
    with pytest.raises(ValueError, match="normal_lambda"):
        T.train_scene(model, scene, [img], 1, normals=[prior], normal_lambda=-1.0)
    assert model.step == 0


def test_autograd_route_takes_the_op_on_the_rendered_depth(gs):
    """the CPU route of train_step: the term is normal_loss at S = 1 on depth * m, m with the camera's intrinsics and the
    image as the guide, and its gradient reaches the parameters; the batch route is the mean of the same per-camera term"""
    T = gs.training
    model, cam, prior, base, hole, H, W = _trainable(gs)
    img = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(3))
    assert not T.one_call_route(model)
    out = model.get_outputs(cam)
    kw = dict(gt_normal=prior, normal_lambda=0.5, normal_smooth_lambda=0.3, normal_edge_beta=2.0)
    h = T.train_step(model, T.make_optimizers(model), cam, img, 0.0, **kw)
    image_term = float(T.image_loss_torch(out["rgb"], img, 0.0).detach())
    m = hole.reshape(1, H, W)
    acc, K = (out["depth"].detach().reshape(1, H, W) * m), (cam.fx, cam.fy, cam.cx, cam.cy)
    want = float(gs.normal_loss(acc, m, K, prior, img, 0.5, 0.3, 2.0))
    ref = R.reference(acc.numpy(), m.numpy(), K, prior=prior.numpy(), guide=img.numpy(), prior_weight=0.5, smooth_weight=0.3,
                      edge_beta=2.0)
    assert abs(want - ref["loss"]) < 1e-6 and ref["stats"][0] == (H - 4) * (W - 2) and ref["stats"][1] == (H - 4) * (W - 3)
    assert want > 1e-3 and h["loss"] == pytest.approx(image_term + want, abs=1e-6)
    assert float(model.scales.grad.abs().max()) > 0 and float(model.means.grad[:, 2].abs().max()) > 0
    # smoothness alone needs no prior
    model, cam, prior, _, _, _, _ = _trainable(gs)
    h2 = T.train_step(model, T.make_optimizers(model), cam, img, 0.0, normal_smooth_lambda=0.3)
    assert h2["loss"] == pytest.approx(image_term + float(gs.normal_loss(acc, m, K, None, None, 0.0, 0.3)), abs=1e-6)
    # the batch route
    model, cam, prior, _, _, _, _ = _trainable(gs)
    single = model.get_outputs
    model.get_outputs_batch = lambda cams, **k: {key: torch.stack([single(c)[key] for c in cams]) for key in ("rgb", "depth", "accumulation")}
    hb = T.train_step(model, T.make_optimizers(model), [cam, cam], [img, img], 0.0, gt_normal=[prior, prior], normal_lambda=0.5,
                      normal_smooth_lambda=0.3, normal_edge_beta=2.0)
    assert hb["loss"] == pytest.approx(image_term + want, abs=1e-6)


def test_one_call_route_hands_the_sums_to_the_op(gs, monkeypatch):
    """the one-call route with a stand-in frame: train_step passes grad_depth_sums only, the callable returns the normal
    op's gradients for the raw sums — plus the depth term's, prior loss or metric L1, when one is on — and the loss gains
    the op's value"""
    T = gs.training
    model, cam, prior, base, hole, H, W = _trainable(gs)
    monkeypatch.setattr(T, "one_call_route", lambda m: True)
    monkeypatch.setattr(gs.fused, "image_loss_with_grad", lambda rgb, gt, lam: (torch.tensor(0.25), torch.zeros_like(rgb), None))
    S = 3
    g = torch.Generator().manual_seed(8)
    alphas = (torch.rand(S, H, W, generator=g) * 0.9 + 0.1) * hole.reshape(1, H, W)
    depth_acc = alphas * (base + 0.3 * torch.rand(H, W, generator=g))
    img = torch.rand(H, W, 3, generator=g)
    depth_prior = (0.37 * base + 1.9)[..., None]
    seen = {}

    def stand_in(camera, grad_image, grad_depth=None, grad_depth_sums=None):
        seen["keywords"] = (grad_depth is not None, grad_depth_sums is not None)
        grad_image(torch.full((H, W, 3), 0.5))
        seen["grads"] = grad_depth_sums(depth_acc, alphas)
        for p in model.gauss_params().values():
            p.grad = torch.zeros_like(p)
        model.radii = torch.ones(1, model.num_points, dtype=torch.int32)
        return torch.full((H, W, 3), 0.5)

    model.render_and_backward = stand_in
    K = (cam.fx, cam.fy, cam.cx, cam.cy)
    nl, nvd, nva = gs.normal_loss_with_grad(depth_acc, alphas, K, prior, img, 0.5, 0.3, 2.0)
    assert float(nl) > 0 and nvd.any()
    kw = dict(gt_normal=prior, normal_lambda=0.5, normal_smooth_lambda=0.3, normal_edge_beta=2.0)
    h = T.train_step(model, T.make_optimizers(model, fused=False), cam, img, 0.2, **kw)
    assert seen["keywords"] == (False, True)
    assert torch.equal(seen["grads"][0], nvd) and torch.equal(seen["grads"][1], nva)
    assert h["loss"] == pytest.approx(0.25 + float(nl), abs=1e-6)
    # with the depth-prior term: the two gradients are added
    h = T.train_step(model, T.make_optimizers(model, fused=False), cam, img, 0.2, gt_depth=depth_prior, depth_lambda=0.5,
                     depth_loss="pearson", **kw)
    dl, dvd, dva = gs.depth_prior_loss_with_grad(depth_acc, alphas, depth_prior.reshape(H, W), "pearson", "depth", 0.5)
    assert seen["keywords"] == (False, True)
    assert torch.equal(seen["grads"][0], dvd + nvd) and torch.equal(seen["grads"][1], dva + nva)
    assert h["loss"] == pytest.approx(0.25 + float(nl) + float(dl), abs=1e-6)
    # with the metric L1: its chain is built inside the same callable, grad_depth is never passed
    h = T.train_step(model, T.make_optimizers(model, fused=False), cam, img, 0.2, gt_depth=depth_prior, depth_lambda=0.5, **kw)
    a, b = depth_acc.clone().requires_grad_(True), alphas.clone().requires_grad_(True)
    ml = T.depth_loss(gs.model.expected_depth(a, b), depth_prior, 0.5)
    ml.backward()
    assert seen["keywords"] == (False, True)
    assert torch.allclose(seen["grads"][0], a.grad + nvd, rtol=0, atol=1e-9) and torch.allclose(seen["grads"][1], b.grad + nva, rtol=0, atol=1e-9)
    assert h["loss"] == pytest.approx(0.25 + float(nl) + float(ml.detach()), abs=1e-6)
    # smoothness alone: no prior reaches the op
    h = T.train_step(model, T.make_optimizers(model, fused=False), cam, img, 0.2, normal_smooth_lambda=0.3)
    sl, svd, _ = gs.normal_loss_with_grad(depth_acc, alphas, K, None, None, 0.0, 0.3)
    assert torch.equal(seen["grads"][0], svd) and h["loss"] == pytest.approx(0.25 + float(sl), abs=1e-6)


def test_downscale_normals(gs):
    T = gs.training
    n = torch.zeros(4, 6, 3)
    n[0:2, 0:2] = torch.tensor([0.0, 0.0, -1.0])                          # a full block
    n[0, 2], n[1, 3] = torch.tensor([0.0, 0.6, -0.8]), torch.tensor([0.0, -0.6, -0.8])     # two valid of four: their mean
    n[2, 0], n[2, 1] = torch.tensor([1.0, 0.0, 0.0]), torch.tensor([-1.0, 0.0, 0.0])       # they cancel
    n[3, 4] = torch.tensor([float("nan"), 0.0, -1.0])                     # not a value
    n[2, 5] = torch.tensor([0.0, 3.0, -4.0])                              # not a unit vector
    out = T.downscale_normals(n, 2)
    assert out.shape == (2, 3, 3) and T.downscale_normals(n, 1) is n
    assert torch.equal(out[0, 0], torch.tensor([0.0, 0.0, -1.0])) and torch.equal(out[0, 1], torch.tensor([0.0, 0.0, -1.0]))
    assert torch.equal(out[1, 0], torch.zeros(3)) and torch.equal(out[0, 2], torch.zeros(3))
    assert torch.allclose(out[1, 2], torch.tensor([0.0, 0.6, -0.8]), atol=1e-6)


# --------------------------------------------------------------------------- #
# the loaders
# --------------------------------------------------------------------------- #
def _write_png16(path, arr):
    """a 16-bit RGB PNG of arr uint16 [H,W,3]; rows filtered None, Sub, Up, Average, Paeth in turn"""
    H, W, _ = arr.shape
    raw = arr.astype(">u2").tobytes()
    stride, bpp = W * 6, 6
    rows = [np.frombuffer(raw[y * stride:(y + 1) * stride], np.uint8).astype(np.int64) for y in range(H)]
    body = b""
    for y, row in enumerate(rows):
        up = rows[y - 1] if y else np.zeros(stride, np.int64)
        left = np.concatenate([np.zeros(bpp, np.int64), row[:-bpp]])
        upleft = np.concatenate([np.zeros(bpp, np.int64), up[:-bpp]])
        ft = y % 5
        if ft == 4:
            pa, pb, pc = np.abs(up - upleft), np.abs(left - upleft), np.abs(left + up - 2 * upleft)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
        else:
            pred = (0, left, up, (left + up) // 2)[ft]
        body += bytes([ft]) + ((row - pred) & 255).astype(np.uint8).tobytes()

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 16, 2, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(body)) + chunk(b"IEND", b""))


def test_loaders_read_both_file_kinds_and_conventions(gs, tmp_path):
    import json
    from PIL import Image
    D = gs.data
    rng = np.random.default_rng(1)
    H, W = 7, 9
    n = rng.standard_normal((H, W, 3)).astype(np.float32)
    n[2, 3] = np.nan
    np.save(tmp_path / "n.npy", n)
    got = D.load_normal(str(tmp_path / "n.npy"))
    want = n.copy()
    want[2, 3] = 0.0
    assert got.dtype == torch.float32 and torch.equal(got, torch.from_numpy(want))
    gl = D.load_normal(str(tmp_path / "n.npy"), "opengl")
    assert torch.equal(gl, torch.from_numpy(want * np.float32([1, -1, -1])))
    with pytest.raises(ValueError, match="normal_convention"):
        D.load_normal(str(tmp_path / "n.npy"), "directx")
    v8 = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    Image.fromarray(v8).save(tmp_path / "n8.png")
    assert torch.equal(D.load_normal(str(tmp_path / "n8.png")), torch.from_numpy((2.0 * v8 / 255.0 - 1.0).astype(np.float32)))
    v16 = rng.integers(0, 65536, (H, W, 3)).astype(np.uint16)
    _write_png16(tmp_path / "n16.png", v16)
    assert torch.equal(D.load_normal(str(tmp_path / "n16.png")), torch.from_numpy((2.0 * v16 / 65535.0 - 1.0).astype(np.float32)))
    np.save(tmp_path / "bad.npy", np.zeros((H, W)))
    with pytest.raises(ValueError, match=r"\[H,W,3\]"):
        D.load_normal(str(tmp_path / "bad.npy"))
    # transforms.json: normal_file_path per frame, normal_convention at the top
    frames = [{"file_path": f"im{i}.npy", "transform_matrix": np.eye(4).tolist()} for i in range(2)]
    frames[1]["normal_file_path"] = "n.npy"
    meta = {"w": W, "h": H, "fl_x": 8.0, "fl_y": 8.0, "cx": 4.5, "cy": 3.5, "frames": frames}
    for conv in (None, "opengl"):
        (tmp_path / "transforms.json").write_text(json.dumps(dict(meta, **({"normal_convention": conv} if conv else {}))))
        scene = D.load_transforms(str(tmp_path))
        assert scene.normal_convention == (conv or "opencv") and scene.normal_paths == [None, str(tmp_path / "n.npy")]
        maps = D.load_scene_normals(scene)
        assert maps[0] is None and torch.equal(maps[1], gl if conv else got)
    (tmp_path / "transforms.json").write_text(json.dumps(dict(meta, normal_convention="directx")))
    with pytest.raises(ValueError, match="normal_convention"):
        D.load_transforms(str(tmp_path))
    assert D.TransformsScene([], [], [], [], 0.0, 0.0).normal_paths == []
    # a lens: nearest-neighbour, cropped like the depth maps
    (tmp_path / "transforms.json").write_text(json.dumps(dict(meta, k1=0.1)))
    scene = D.load_transforms(str(tmp_path))
    np.save(tmp_path / "d.npy", np.ones((H, W), np.float32))
    scene.depth_paths = [None, str(tmp_path / "d.npy")]
    nm, dm = D.load_scene_normals(scene)[1], D.load_scene_depths(scene)[1]
    assert nm.shape[:2] == dm.shape[:2] and nm.shape[0] <= H
    flat = {tuple(v) for v in want.reshape(-1, 3).tolist()}
    assert all(tuple(v) in flat for v in nm.reshape(-1, 3).tolist())         # every vector is one of the source's, unrotated


# --------------------------------------------------------------------------- #
# the C ABI, the tools' flags
# --------------------------------------------------------------------------- #
def test_abi_entries(gs):
    lib_mod = gs._lib
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "gsdeblur.h").read_text(), flags=re.S)
    for name, n_args in NEW_EXPORTS.items():
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m and len([a for a in m.group(1).split(",") if a.strip()]) == n_args, name
        sigs = lib_mod._SIGS if name in lib_mod._SIGS else lib_mod._SIGS_LL
        assert len(sigs[name]) == n_args
        assert name in (ROOT / "INTEGRATION.md").read_text()
    from gsdeblur_amd import _build
    assert dict(_build.SOURCES)["normals.hip"] == ["-ffp-contract=off"]
    lib = lib_mod.load()
    ws = lib.gs_normal_loss_workspace_bytes
    groups_1080p = -(-1920 // (TW * GROUP)) * -(-1080 // TH)
    assert ws(1, 5, 1080, 1920) == groups_1080p * 48 + 1080 * 1920 * 20 and ws(3, 5, 1080, 1920) == 3 * ws(1, 5, 1080, 1920)
    assert ws(0, 1, 4, 4) == 0 and ws(1, 1, 1, 1) == 48 + 20
    assert ws(1, 0, 4, 4) == -1 and ws(1, 1, 0, 4) == -1 and ws(-1, 1, 4, 4) == -1
    assert ws(2, 129, 4, 4) == -1 and ws(256, 1, 4, 4) > 0                    # B * S <= 256
    assert ws(1, 1, 1 << 15, 1 << 15) == -1 and ws(1, 4, 1 << 14, 1 << 14) == -1 and ws(1, 3, 1 << 14, 1 << 14) > 0
    call, fwd = lib.gs_normal_loss, lib.gs_depth_normals
    null = None
    tail = (null, null, null, null, null, null, 0, null)
    assert call(0, 1, 4, 4, null, null, null, null, null, 1.0, 0.0, 0.0, 0.0, *tail) == 0
    assert call(1, 1, 4, 4, null, null, null, null, null, 1.0, 0.0, 0.0, 0.0, *tail) == 1     # null pointers
    assert call(1, 0, 4, 4, null, null, null, null, null, 1.0, 0.0, 0.0, 0.0, *tail) == 1
    assert call(2, 129, 4, 4, null, null, null, null, null, 1.0, 0.0, 0.0, 0.0, *tail) == 1
    assert call(0, 1, 4, 4, null, null, null, null, null, 1.0, 0.0, -1.0, 0.0, *tail) == 1    # edge_beta < 0
    assert call(0, 1, 4, 4, null, null, null, null, null, 1.0, 0.0, 0.0, -0.5, *tail) == 1    # min_alpha < 0
    assert call(0, 1, 4, 4, null, null, null, null, null, float("nan"), 0.0, 0.0, 0.0, *tail) == 1
    assert fwd(0, 1, 4, 4, null, null, null, 0.0, null, null) == 0
    assert fwd(1, 1, 4, 4, null, null, null, 0.0, null, null) == 1 and fwd(0, 1, 4, 4, null, null, null, -1.0, null, null) == 1


def test_tool_flags_parse():
    import importlib
    ap = importlib.import_module("train_deblur").build_parser()
    a = ap.parse_args([])
    assert (a.normal_lambda, a.normal_smooth_lambda, a.normal_edge_beta) == (0.0, 0.0, 0.0)
    a = ap.parse_args(["--normal-lambda", "0.05", "--normal-smooth-lambda", "0.01", "--normal-edge-beta", "4"])
    assert (a.normal_lambda, a.normal_smooth_lambda, a.normal_edge_beta) == (0.05, 0.01, 4.0)
    assert "normal_file_path" in ap.format_help()
    tool = importlib.import_module("render_model")
    ap = tool.build_parser()
    base = ["--ply", "m.ply", "--data", "d", "--out", "o"]
    assert ap.parse_args(base).normals is False and ap.parse_args(base + ["--normals"]).normals is True
    pic = tool.normal_picture(torch.tensor([[[0.0, 0.0, -1.0], [0.0, 0.0, 0.0], [0.6, 0.8, 0.0]]]))
    assert torch.allclose(pic, torch.tensor([[[0.5, 0.5, 1.0], [0.0, 0.0, 0.0], [0.8, 0.1, 0.5]]]))
