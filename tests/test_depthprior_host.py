"""The depth-prior loss on the CPU: csrc/depthprior_math.h compiled with g++ and depth_prior_loss_torch against the float64
reference (tests/depthprior_reference.py, whose docstring states the tolerance rule); the reference's gradient against
float64 autograd of a plain 1 - corrcoef and of a masked L1; known answers, the degenerate rule, scale and shift
invariance; the training surface with a stand-in render; the C-ABI entries and the trainer's flags."""
import ctypes
import re
import subprocess
import types
from pathlib import Path

import numpy as np
import pytest
import torch

import depthprior_reference as R

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "host_math" / "depthprior_host.cpp"
LIB = ROOT / "tests" / "host_math" / "libdepthprior_host.so"
CSRC = ROOT / "3dgs-deblur_amd" / "csrc"
HDR = CSRC / "depthprior_math.h"
HIP = CSRC / "depthprior.hip"
NEW_EXPORTS = {"gs_depth_prior_workspace_bytes": 4, "gs_depth_prior_loss": 18}


def kernel_constant(name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, HIP.read_text()).group(1))


K_TILE, K_THREADS = kernel_constant("kTile"), kernel_constant("kThreads")
SIZES = [(1, 1), (2, 1), (7, 13), (67, 131), (1, K_TILE - 1), (1, K_TILE), (1, K_TILE + 1)]
MANY_TILES = (1, K_TILE * K_THREADS + 1)          # more tile records than the gradient kernel's workgroup has threads


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def dph():
    if not LIB.exists() or LIB.stat().st_mtime < max(f.stat().st_mtime for f in (SRC, HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", f"-I{CSRC}", str(SRC),
                               "-o", str(LIB)])
    lib = ctypes.CDLL(str(LIB))
    lib.dph_degenerate_tol.restype = ctypes.c_double
    lib.dph_depth_prior_loss.restype = None
    lib.dph_depth_prior_loss.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p] * 3 + [ctypes.c_int] * 2 + \
        [ctypes.c_float] * 2 + [ctypes.c_void_p] * 4
    return lib


def host_loss(lib, acc, al, pr, kind, space, weight=1.0, min_alpha=0.0):
    """the host-compiled header on [B,S,H,W] arrays -> loss [B], stats [B,8], v_depth_acc, v_alphas"""
    acc, al, pr = (np.ascontiguousarray(t, np.float32) for t in (acc, al, pr))
    B, S, H, W = acc.shape
    loss, stats = np.empty(B, np.float32), np.empty((B, 8), np.float64)
    vd, va = np.empty_like(acc), np.empty_like(al)
    lib.dph_depth_prior_loss(B, S, H, W, P(acc), P(al), P(pr), R.KINDS.index(kind), R.SPACES.index(space), min_alpha, weight,
                             P(loss), P(stats), P(vd), P(va))
    return loss, stats, vd, va


def torch_loss(gs, acc, al, pr, kind, space, weight=1.0, min_alpha=0.0):
    out = gs.depthprior.depth_prior_loss_torch(torch.from_numpy(acc), torch.from_numpy(al), torch.from_numpy(pr), kind, space,
                                               weight, min_alpha, return_stats=True)
    return tuple(t.numpy() for t in out)


# --------------------------------------------------------------------------- #
# the op against the reference
# --------------------------------------------------------------------------- #
def test_constants_agree(gs, dph):
    D = gs.depthprior
    assert dph.dph_moments() == 7 and dph.dph_stats() == D.STATS == 8
    assert dph.dph_degenerate_tol() == D.DEGENERATE_TOL == R.DEGENERATE_TOL
    assert D.KINDS == R.KINDS and D.SPACES == R.SPACES
    assert K_TILE % K_THREADS == 0 and K_TILE >= 2


# the large size at S = 1, B = 1 only here; the GPU tests run every combination
HOST_CASES = [(size, S, B) for size in SIZES for S, B in ((1, 1), (5, 3))] + [(MANY_TILES, 1, 1)]


@pytest.mark.parametrize("size,S,B", HOST_CASES, ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v))
def test_header_and_torch_restatement_match_the_reference(gs, dph, size, S, B):
    H, W = size
    for space in R.SPACES:
        acc, al, pr, priors = R.make_batch(B, S, H, W, space, seed=11 + H + W)
        for b in range(B):
            R.assert_input_conditions(acc[b], al[b], pr[b], space, expect_degenerate=priors[b] != "noisy" or H * W < 2)
        for kind in R.KINDS:
            h = host_loss(dph, acc, al, pr, kind, space, weight=0.7)
            t_loss, t_vd, t_va, t_stats = torch_loss(gs, acc, al, pr, kind, space, weight=0.7)
            for b in range(B):
                what = (kind, space, S, b, size)
                R.check_frame(h[0][b], h[2][b], h[3][b], acc[b], al[b], pr[b], kind, space, 0.7, what=("header",) + what)
                R.check_frame(t_loss[b], t_vd[b], t_va[b], acc[b], al[b], pr[b], kind, space, 0.7, what=("torch",) + what)
                ref = R.reference(acc[b], al[b], pr[b], kind, space, 0.7)
                for got in (h[1][b], t_stats[b]):
                    assert got[0] == ref["stats"][0]                                  # the same pixels took part
                    # float64 sums of n non-negative terms in two orders: within n ulps of each other (rho, entry 7,
                    # is what the loss check above covers)
                    assert np.allclose(got[:7], ref["stats"][:7], rtol=max(H * W, 1) * 2.0 ** -52, atol=0)


@pytest.mark.parametrize("size", [(7, 13), (67, 131)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("space", R.SPACES)
def test_reference_gradient_is_float64_autograd_of_plain_torch(size, S, space):
    """reference(store=None) is all float64, and so is autograd of 1 - corrcoef / a masked L1 on the same numbers: they
    differ by float64 rounding alone (1e-9 relative leaves six digits of room)"""
    H, W = size
    acc, al, pr, _ = R.make_frame(S, H, W, space, seed=5)
    for kind in R.KINDS:
        ref = R.reference(acc, al, pr, kind, space, 0.7, store=None)
        a64 = torch.from_numpy(acc).double().requires_grad_(True)
        l64 = torch.from_numpy(al).double().requires_grad_(True)
        d, a = a64.sum(0) / S, l64.sum(0) / S
        valid = torch.from_numpy(ref["valid"])
        x = (d[valid] / a[valid]) if space == "depth" else (a[valid] / d[valid])
        y = torch.from_numpy(pr).double()[valid]
        w = float(np.float32(0.7))
        loss = w * (1.0 - torch.corrcoef(torch.stack([x, y]))[0, 1]) if kind == "pearson" else w * (x - y).abs().mean()
        loss.backward()
        assert abs(float(loss.detach()) - ref["loss"]) < 1e-12
        for got, want in ((ref["v_depth_acc"], a64.grad.numpy()), (ref["v_alphas"], l64.grad.numpy())):
            assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()


# --------------------------------------------------------------------------- #
# known answers, the degenerate rule, invariance
# --------------------------------------------------------------------------- #
def _exact_depth(H=23, W=31, seed=4):
    """one sample, alpha 1: x is the depth itself"""
    depth = np.random.default_rng(seed).uniform(2.0, 8.0, (H, W)).astype(np.float32)
    return depth[None], np.ones((1, H, W), np.float32), depth


def both(gs, dph, acc, al, pr, kind, space, weight=1.0):
    """(loss, v_depth_acc, v_alphas) of one frame from the host-compiled header and from the torch restatement"""
    h = host_loss(dph, acc[None], al[None], pr[None], kind, space, weight)
    t = torch_loss(gs, acc, al, pr, kind, space, weight)
    return (h[0][0], h[2][0], h[3][0]), (t[0], t[1], t[2])


def test_known_answers(gs, dph):
    acc, al, depth = _exact_depth()
    cases = [("depth", (3.0 * depth + 2.0).astype(np.float32), 0.0),
             ("disparity", (2.0 / depth + 0.1).astype(np.float32), 0.0),
             ("depth", (30.0 - 3.0 * depth).astype(np.float32), 2.0)]          # a negated prior: rho = -1
    for space, pr, want in cases:
        _, tol, _ = R.tolerances(acc, al, pr, "pearson", space, 0.5)
        for loss, _, _ in both(gs, dph, acc, al, pr, "pearson", space, 0.5):
            assert abs(float(loss) - want * 0.5) <= tol, (space, want, float(loss), tol)
    # l1: prior = depth + 0.25 exactly (multiples of 2^-10 keep the sum exact)
    q = np.round(depth * 1024) / 1024
    for loss, vd, _ in both(gs, dph, q[None].astype(np.float32), al, (q + 0.25).astype(np.float32), "l1", "depth", 0.5):
        assert float(loss) == 0.125 and np.all(vd == np.float32(-0.5 / q.size))


def test_degenerate_frames_give_exact_zeros(gs, dph):
    acc, al, depth = _exact_depth()
    pr = (3.0 * depth + 2.0).astype(np.float32)
    one = np.zeros_like(pr)
    one[3, 4] = 1.0
    const_render = np.full_like(acc, 4.0)
    for name, a, p in (("n=0", acc, np.zeros_like(pr)), ("n=1", acc, one), ("constant prior", acc, np.full_like(pr, 1.5)),
                       ("constant render", const_render, pr)):
        for space in R.SPACES:
            for loss, vd, va in both(gs, dph, a, al, p, "pearson", space):
                assert float(loss) == 0.0 and not vd.any() and not va.any(), (name, space)
    for loss, vd, va in both(gs, dph, acc, al, np.zeros_like(pr), "l1", "depth"):
        assert float(loss) == 0.0 and not vd.any() and not va.any()


def test_invalid_pixels_get_exact_zeros(gs, dph):
    for space in R.SPACES:
        acc, al, pr, _ = R.make_frame(5, 33, 47, space, seed=9)
        al2 = al.copy()
        al2[:, 5] *= 0.01                      # a row below min_alpha = 0.02
        for kind in R.KINDS:
            ref = R.reference(acc, al2, pr, kind, space, 1.0, 0.02)
            assert 0 < ref["valid"].sum() < ref["valid"].size and not ref["valid"][5].any()
            h = host_loss(dph, acc[None], al2[None], pr[None], kind, space, 1.0, 0.02)
            t = torch_loss(gs, acc, al2, pr, kind, space, 1.0, 0.02)
            for vd, va in ((h[2][0], h[3][0]), (t[1], t[2])):
                dead = ~np.broadcast_to(ref["valid"], vd.shape)
                assert not vd[dead].any() and not va[dead].any()
                assert vd[~dead].all() or kind == "l1"
            R.check_frame(h[0][0], h[2][0], h[3][0], acc, al2, pr, kind, space, 1.0, 0.02)


def test_scale_invariance_is_bit_exact(gs, dph):
    """every operation of the Pearson loss commutes with a power of two: a prior times 4 changes no bit"""
    for space in R.SPACES:
        acc, al, pr, _ = R.make_frame(5, 67, 131, space, seed=21)
        for one, four in zip(both(gs, dph, acc, al, pr, "pearson", space, 0.7),
                             both(gs, dph, acc, al, (pr * 4).astype(np.float32), "pearson", space, 0.7)):
            for a, b in zip(one, four):
                assert np.array_equal(a, b)
            assert float(one[0]) > 0 and one[1].any()


def test_shift_invariance(gs, dph):
    """a prior of multiples of 2^-10 in [1, 8) plus 8.0 is still exact in float32: the loss moves by less than 1e-6"""
    rng = np.random.default_rng(3)
    for space in R.SPACES:
        acc, al, pr, _ = R.make_frame(5, 67, 131, space, seed=22)
        q = (rng.integers(1 << 10, 8 << 10, pr.shape) / 1024.0).astype(np.float32)
        q[pr == 0] = 0.0
        shifted = np.where(q > 0, q + np.float32(8.0), 0).astype(np.float32)
        assert np.array_equal(shifted[q > 0].astype(np.float64), q[q > 0].astype(np.float64) + 8.0)
        for one, two in zip(both(gs, dph, acc, al, q, "pearson", space), both(gs, dph, acc, al, shifted, "pearson", space)):
            print(space, float(one[0]), float(two[0]))
            assert abs(float(one[0]) - float(two[0])) < 1e-6


# --------------------------------------------------------------------------- #
# the Python surface
# --------------------------------------------------------------------------- #
def test_argument_checks(gs):
    D = gs.depthprior
    acc, al, pr = torch.rand(2, 4, 5), torch.rand(2, 4, 5) + 0.1, torch.rand(4, 5) + 0.1
    for fn in (gs.depth_prior_loss, gs.depth_prior_loss_with_grad, D.depth_prior_loss_torch):
        with pytest.raises(ValueError, match="kind"):
            fn(acc, al, pr, kind="huber")
        with pytest.raises(ValueError, match="space"):
            fn(acc, al, pr, space="log")
        with pytest.raises(ValueError, match="float32"):
            fn(acc.double(), al, pr)
        with pytest.raises(ValueError, match="prior must be"):
            fn(acc, al, pr[None])
        with pytest.raises(ValueError, match="alphas must have"):
            fn(acc, al[:1], pr)
        with pytest.raises(ValueError, match="min_alpha"):
            fn(acc, al, pr, min_alpha=-0.1)
        with pytest.raises(ValueError):
            fn(acc[0], al[0], pr)
        with pytest.raises(ValueError, match="B \\* S"):
            fn(torch.rand(2, 129, 1, 1), torch.rand(2, 129, 1, 1), torch.rand(2, 1, 1))
    with pytest.raises(ValueError, match="HIP"):
        D.depth_prior_loss_hip(acc[None], al[None], pr[None])
    assert gs.depth_prior_loss is D.depth_prior_loss and gs.depth_prior_loss_with_grad is D.depth_prior_loss_with_grad


def test_autograd_function_on_the_cpu(gs):
    acc, al, pr, _ = R.make_batch(2, 3, 9, 11, "depth", seed=2)
    acc, al, pr = torch.from_numpy(acc), torch.from_numpy(al), torch.from_numpy(pr)
    loss, vd, va = gs.depth_prior_loss_with_grad(acc, al, pr, weight=0.7)
    assert loss.shape == (2,) and vd.shape == acc.shape
    a, b = acc.clone().requires_grad_(True), al.clone().requires_grad_(True)
    out = gs.depth_prior_loss(a, b, pr, weight=0.7)
    assert torch.equal(out.detach(), loss)
    (out * torch.tensor([1.0, 0.5])).sum().backward()
    assert torch.equal(a.grad[0], vd[0]) and torch.equal(a.grad[1], vd[1] * 0.5)
    assert torch.equal(b.grad[0], va[0]) and torch.equal(b.grad[1], va[1] * 0.5)
    # a single frame: a scalar, and the frame of a batch alone gives the batch's bits
    l0, vd0, va0 = gs.depth_prior_loss_with_grad(acc[1], al[1], pr[1], weight=0.7)
    assert l0.shape == () and torch.equal(l0, loss[1]) and torch.equal(vd0, vd[1]) and torch.equal(va0, va[1])


# --------------------------------------------------------------------------- #
# the training surface, with a stand-in render on the CPU
# --------------------------------------------------------------------------- #
TH, TW = 12, 16


def _cpu_trainable(gs, n=30):
    g = torch.Generator().manual_seed(3)
    cfg = gs.SplatfactoDeblurConfig(sh_degree=1)
    model = gs.SplatfactoDeblurModel(cfg, torch.randn(n, 3, generator=g), torch.zeros(n, 3), torch.randn(n, 4, generator=g),
                                     torch.zeros(n), torch.rand(n, 3, generator=g), torch.zeros(n, 3, 3), num_cameras=2)
    base = torch.rand(TH, TW, generator=g) * 4 + 2
    pattern = torch.rand(TH, TW, generator=g)
    hole = torch.zeros(TH, TW, 1)
    hole[2:, :] = 1.0                                    # the first two rows are not covered

    def fake_outputs(camera, **kw):
        model.radii = torch.ones(1, model.num_points, dtype=torch.int32)
        rgb = model.features_dc.mean(0)[None, None, :].expand(TH, TW, 3)
        # not affine in base: the Pearson loss ignores a scale and a shift of the whole map
        depth = (base + pattern * (1.0 + model.means[:, 2].mean() + model.scales.sum()))[..., None]
        return {"rgb": rgb, "depth": torch.where(hole > 0, depth, depth.detach().max()), "accumulation": hole}

    model.get_outputs = fake_outputs
    cam = gs.Camera(torch.eye(4)[:3], 10.0, 10.0, 8.0, 6.0, TW, TH, metadata={"cam_idx": 0})
    prior = (0.37 * base + 1.9 + 0.3 * torch.rand(TH, TW, generator=g))[..., None]
    prior[:, 3] = 0.0
    return model, cam, prior, base, hole


def test_train_step_rejects_unknown_names_before_anything_runs(gs):
    T = gs.training
    model, cam, prior, _, _ = _cpu_trainable(gs)
    model.get_outputs = lambda *a, **k: pytest.fail("rendered before the names were checked")
    opts = T.make_optimizers(model)
    img = torch.full((TH, TW, 3), 0.5)
    with pytest.raises(ValueError, match="depth_loss"):
        T.train_step(model, opts, cam, img, gt_depth=prior, depth_lambda=0.1, depth_loss="huber")
    with pytest.raises(ValueError, match="depth_space"):
        T.train_step(model, opts, cam, img, gt_depth=prior, depth_lambda=0.1, depth_loss="pearson", depth_space="log")
    with pytest.raises(ValueError, match="depth_loss"):
        T.train_step(model, opts, [cam], [img], gt_depth=[prior], depth_lambda=0.1, depth_loss="huber")
    scene = types.SimpleNamespace(cameras=[cam], train_indices=[0], eval_indices=[0])
    with pytest.raises(ValueError, match="depth_space"):
        T.train_scene(model, scene, [img], 1, depths=[prior], depth_lambda=0.1, depth_loss="l1", depth_space="log")
    assert model.step == 0


@pytest.mark.parametrize("kind", ["pearson", "l1"])
def test_autograd_route_takes_the_op_on_the_rendered_depth(gs, kind):
    """the CPU route of train_step: the depth term is depth_prior_loss at S = 1 on depth * m, m (x = depth exactly), its
    gradient reaches the parameters, and depth_loss=None is still the metric L1"""
    T = gs.training
    img = torch.full((TH, TW, 3), 0.5)
    losses = {}
    for dl in (None, kind):
        model, cam, prior, base, hole = _cpu_trainable(gs)
        assert not T.one_call_route(model)
        out = model.get_outputs(cam)
        h = T.train_step(model, T.make_optimizers(model), cam, img, 0.0, gt_depth=prior, depth_lambda=0.5, depth_loss=dl)
        image_term = float(T.image_loss_torch(out["rgb"], img, 0.0).detach())
        if dl is None:
            want = float(T.depth_loss(out["depth"], prior, 0.5))
        else:
            m = hole.reshape(1, TH, TW)
            want = float(gs.depth_prior_loss(out["depth"].detach().reshape(1, TH, TW) * m, m, prior.reshape(TH, TW), kind,
                                             "depth", 0.5))
            ref = R.reference((out["depth"].detach().reshape(1, TH, TW) * m).numpy(), m.numpy(), prior.reshape(TH, TW).numpy(),
                              kind, "depth", 0.5)
            assert abs(want - ref["loss"]) < 1e-6 and ref["valid"].sum() == (TH - 2) * (TW - 1)
        assert h["loss"] == pytest.approx(image_term + want, abs=1e-6)
        assert float(model.scales.grad.abs().max()) > 0 and float(model.means.grad[:, 2].abs().max()) > 0
        losses[dl] = want
    assert losses[None] != losses[kind]
    # the batch route: the mean over the cameras of the same per-camera term
    model, cam, prior, _, _ = _cpu_trainable(gs)
    single = model.get_outputs
    model.get_outputs_batch = lambda cams, **kw: {k: torch.stack([single(c)[k] for c in cams]) for k in ("rgb", "depth", "accumulation")}
    h = T.train_step(model, T.make_optimizers(model), [cam, cam], [img, img], 0.0, gt_depth=[prior, prior], depth_lambda=0.5,
                     depth_loss=kind)
    assert h["loss"] == pytest.approx(image_term + losses[kind], abs=1e-6)


def test_one_call_route_hands_the_sums_to_the_op(gs, monkeypatch):
    """the one-call route with a stand-in frame: train_step passes grad_depth_sums (not grad_depth), the callable returns
    depth_prior_loss_with_grad's two gradients for the raw sums, and the loss gains the op's value"""
    T = gs.training
    model, cam, prior, base, hole = _cpu_trainable(gs)
    monkeypatch.setattr(T, "one_call_route", lambda m: True)
    monkeypatch.setattr(gs.fused, "image_loss_with_grad", lambda rgb, gt, lam: (torch.tensor(0.25), torch.zeros_like(rgb), None))
    S = 3
    g = torch.Generator().manual_seed(8)
    alphas = (torch.rand(S, TH, TW, generator=g) * 0.9 + 0.1) * hole.reshape(1, TH, TW)
    depth_acc = alphas * base
    seen = {}

    def stand_in(camera, grad_image, grad_depth=None, grad_depth_sums=None):
        seen["keywords"] = (grad_depth is not None, grad_depth_sums is not None)
        grad_image(torch.full((TH, TW, 3), 0.5))
        seen["grads"] = grad_depth_sums(depth_acc, alphas)
        for p in model.gauss_params().values():
            p.grad = torch.zeros_like(p)
        model.radii = torch.ones(1, model.num_points, dtype=torch.int32)
        return torch.full((TH, TW, 3), 0.5)

    model.render_and_backward = stand_in
    h = T.train_step(model, T.make_optimizers(model, fused=False), cam, torch.full((TH, TW, 3), 0.5), 0.2, gt_depth=prior,
                     depth_lambda=0.5, depth_loss="pearson", depth_space="disparity")
    assert seen["keywords"] == (False, True)
    loss, vd, va = gs.depth_prior_loss_with_grad(depth_acc, alphas, prior.reshape(TH, TW), "pearson", "disparity", 0.5)
    assert torch.equal(seen["grads"][0], vd) and torch.equal(seen["grads"][1], va) and float(loss) > 0
    assert h["loss"] == pytest.approx(0.25 + float(loss), abs=1e-6)
    # depth_loss=None keeps the metric route: grad_depth, no grad_depth_sums
    def metric_stand_in(camera, grad_image, grad_depth=None, grad_depth_sums=None):
        seen["keywords"] = (grad_depth is not None, grad_depth_sums is not None)
        grad_image(torch.full((TH, TW, 3), 0.5))
        grad_depth(torch.full((TH, TW, 1), 3.0), hole)
        for p in model.gauss_params().values():
            p.grad = torch.zeros_like(p)
        return torch.full((TH, TW, 3), 0.5)

    model.render_and_backward = metric_stand_in
    T.train_step(model, T.make_optimizers(model, fused=False), cam, torch.full((TH, TW, 3), 0.5), 0.2, gt_depth=prior,
                 depth_lambda=0.5)
    assert seen["keywords"] == (True, False)


def test_render_and_backward_rejects_both_depth_keywords(gs):
    model, cam, _, _, _ = _cpu_trainable(gs)
    with pytest.raises(ValueError, match="not both"):
        model.render_and_backward(cam, lambda rgb: rgb, grad_depth=lambda d, a: d, grad_depth_sums=lambda d, a: (d, a))


# --------------------------------------------------------------------------- #
# the C ABI, the trainer's flags
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
    F, I, P_, L = ctypes.c_float, ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong
    assert lib_mod._SIGS["gs_depth_prior_loss"] == [I] * 4 + [P_] * 3 + [I, I, F, F] + [P_] * 5 + [L, P_]
    from gsdeblur_amd import _build
    assert dict(_build.SOURCES)["depthprior.hip"] == ["-ffp-contract=off"]
    lib = lib_mod.load()
    ws = lib.gs_depth_prior_workspace_bytes
    tiles_1080p = -(-1080 * 1920 // K_TILE)
    assert ws(1, 5, 1080, 1920) == tiles_1080p * 56 and ws(3, 5, 1080, 1920) == 3 * tiles_1080p * 56
    assert ws(0, 1, 4, 4) == 0 and ws(1, 1, 1, 1) == 56
    assert ws(1, 0, 4, 4) == -1 and ws(1, 1, 0, 4) == -1 and ws(-1, 1, 4, 4) == -1
    assert ws(2, 129, 4, 4) == -1 and ws(256, 1, 4, 4) > 0                    # B * S <= 256
    assert ws(1, 1, 1 << 15, 1 << 15) == -1 and ws(1, 4, 1 << 14, 1 << 14) == -1 and ws(1, 3, 1 << 14, 1 << 14) > 0
    call = lib.gs_depth_prior_loss
    null = None
    assert call(0, 1, 4, 4, null, null, null, 0, 0, 0.0, 1.0, null, null, null, null, null, 0, null) == 0
    assert call(1, 1, 4, 4, null, null, null, 0, 0, 0.0, 1.0, null, null, null, null, null, 0, null) == 1     # null pointers
    assert call(1, 0, 4, 4, null, null, null, 0, 0, 0.0, 1.0, null, null, null, null, null, 0, null) == 1
    assert call(2, 129, 4, 4, null, null, null, 0, 0, 0.0, 1.0, null, null, null, null, null, 0, null) == 1
    assert call(0, 1, 4, 4, null, null, null, 2, 0, 0.0, 1.0, null, null, null, null, null, 0, null) == 1     # unknown kind
    assert call(0, 1, 4, 4, null, null, null, 0, 2, 0.0, 1.0, null, null, null, null, null, 0, null) == 1     # unknown space
    assert call(0, 1, 4, 4, null, null, null, 0, 0, -0.5, 1.0, null, null, null, null, null, 0, null) == 1    # min_alpha < 0


def test_train_deblur_flags_parse():
    import importlib
    tool = importlib.import_module("train_deblur")
    ap = tool.build_parser()
    a = ap.parse_args([])
    assert a.depth_lambda == 0.0 and a.depth_loss is None and a.depth_space == "depth"
    a = ap.parse_args(["--depth-lambda", "0.05", "--depth-loss", "pearson", "--depth-space", "disparity"])
    assert (a.depth_lambda, a.depth_loss, a.depth_space) == (0.05, "pearson", "disparity")
    for bad in (["--depth-loss", "huber"], ["--depth-space", "log"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    help_text = ap.format_help()
    assert "depth_file_path" in help_text and "unit" in help_text
