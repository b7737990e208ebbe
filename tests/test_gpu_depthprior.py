"""The depth-prior loss on the MI355X: the kernels of csrc/depthprior.hip against the float64 reference
(tests/depthprior_reference.py, whose docstring states the tolerance rule), bit-identity, the autograd form, the training
routes, and whether a non-metric prior recovers geometry end to end."""
import functools
import time

import numpy as np
import pytest
import torch

import depthprior_reference as R
from test_depthprior_host import K_THREADS, K_TILE, MANY_TILES, SIZES

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=4)
def _inputs(B, S, H, W, space):
    """the inputs of a shape, made once and shared by its cases (never written)"""
    acc, al, pr, priors = R.make_batch(B, S, H, W, space, seed=11 + H + W)
    for b in range(B):
        R.assert_input_conditions(acc[b], al[b], pr[b], space, expect_degenerate=priors[b] != "noisy" or H * W < 2)
    return acc, al, pr


def _run(gs, dev, acc, al, pr, kind, space, weight=0.7, min_alpha=0.0):
    out = gs.depth_prior_loss_with_grad(torch.from_numpy(acc).to(dev), torch.from_numpy(al).to(dev),
                                        torch.from_numpy(pr).to(dev), kind, space, weight, min_alpha, return_stats=True)
    return tuple(t.cpu().numpy() for t in out)


def test_sizes_cover_what_they_claim():
    assert [s[1] for s in SIZES[-3:]] == [K_TILE - 1, K_TILE, K_TILE + 1]
    assert -(-MANY_TILES[0] * MANY_TILES[1] // K_TILE) > K_THREADS          # the record loop takes a second trip


@pytest.mark.parametrize("kind", R.KINDS)                 # varies fastest: the two kinds of a shape share its inputs
@pytest.mark.parametrize("space", R.SPACES)
@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("size", SIZES + [MANY_TILES], ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernels_match_the_reference(gs, dev, kind, space, S, B, size):
    """loss, both gradients and the moments against the reference under the project's rule (4 x what float32 storage costs
    the reference itself + 1e-6; gradients relative to the frame's largest reference gradient); exact zeros at every
    invalid pixel and for the degenerate frames of the B = 3 batch (an all-zero and a constant prior); every frame of a
    batch bit-identical to that frame alone"""
    H, W = size
    acc, al, pr = _inputs(B, S, H, W, space)
    loss, vd, va, stats = _run(gs, dev, acc, al, pr, kind, space)
    assert loss.shape == (B,) and vd.shape == acc.shape and va.shape == al.shape and stats.shape == (B, 8)
    for b in range(B):
        fig = R.check_frame(loss[b], vd[b], va[b], acc[b], al[b], pr[b], kind, space, 0.7, what=(kind, space, S, b, size))
        ref = R.reference(acc[b], al[b], pr[b], kind, space, 0.7)
        assert stats[b, 0] == ref["stats"][0]
        assert np.allclose(stats[b, :7], ref["stats"][:7], rtol=max(H * W, 1) * 2.0 ** -52, atol=0)
        if b == 0 and H * W > 2:                     # (two pixels correlate perfectly: their gradient is zero)
            assert vd[b].any() and va[b].any() and not ref["degenerate"]
        if B > 1:
            l1, vd1, va1, st1 = _run(gs, dev, acc[b], al[b], pr[b], kind, space)
            assert l1 == loss[b] and np.array_equal(vd1, vd[b]) and np.array_equal(va1, va[b]) and np.array_equal(st1, stats[b])
    print(fig)


def test_min_alpha_leaves_pixels_out(gs, dev):
    acc, al, pr, _ = R.make_frame(5, 67, 131, "depth", seed=9)
    al = al.copy()
    al[:, 5] *= 0.01
    for kind in R.KINDS:
        loss, vd, va, stats = _run(gs, dev, acc, al, pr, kind, "depth", 1.0, 0.02)
        R.check_frame(loss, vd, va, acc, al, pr, kind, "depth", 1.0, 0.02)
        assert not vd[:, 5].any() and vd[:, 6].any()


def test_two_runs_and_a_full_size_call_agree_bit_for_bit(gs, dev):
    """1080p, S = 5: finite, and two runs of the same call give the same bits"""
    S, H, W = 5, 1080, 1920
    g = torch.Generator().manual_seed(4)
    depth = torch.rand(H, W, generator=g) * 6 + 2
    al = torch.rand(S, H, W, generator=g) * 0.9 + 0.1
    al[:, :, :64] = 0.0
    acc, al = (al * depth * (1.0 + 0.05 * torch.randn(S, H, W, generator=g))).to(dev), al.to(dev)
    for kind, space, prior in (("pearson", "disparity", 2.0 / depth + 0.1 + 0.01 * torch.randn(H, W, generator=g)),
                               ("l1", "depth", depth + 0.1 * torch.randn(H, W, generator=g))):
        prior = prior.clamp(min=0.01).to(dev)
        one = gs.depth_prior_loss_with_grad(acc, al, prior, kind, space, 0.3, return_stats=True)
        two = gs.depth_prior_loss_with_grad(acc, al, prior, kind, space, 0.3, return_stats=True)
        for a, b in zip(one, two):
            assert torch.isfinite(a).all() and torch.equal(a, b)
        assert float(one[0]) > 0 and float(one[3][0]) == H * (W - 64)
        assert not one[1][:, :, :64].any() and one[1][:, :, 64:].any() and one[2][:, :, 64:].any()


def test_autograd_form_and_upstream_gradient(gs, dev):
    acc, al, pr = (torch.from_numpy(t).to(dev) for t in _inputs(3, 5, 67, 131, "depth"))
    loss, vd, va = gs.depth_prior_loss_with_grad(acc, al, pr, "pearson", "depth", 0.7)
    a, b = acc.clone().requires_grad_(True), al.clone().requires_grad_(True)
    out = gs.depth_prior_loss(a, b, pr, "pearson", "depth", 0.7)
    assert torch.equal(out.detach(), loss)
    out.sum().backward()
    assert torch.equal(a.grad, vd) and torch.equal(b.grad, va)
    a.grad = b.grad = None
    (gs.depth_prior_loss(a, b, pr, "pearson", "depth", 0.7) * 0.5).sum().backward()
    assert torch.equal(a.grad, vd * 0.5) and torch.equal(b.grad, va * 0.5)
    # one frame: a scalar
    a1 = acc[0].clone().requires_grad_(True)
    s = gs.depth_prior_loss(a1, al[0], pr[0], "pearson", "depth", 0.7)
    assert s.shape == () and torch.equal(s.detach(), loss[0])
    s.backward()
    assert torch.equal(a1.grad, vd[0])


def test_hip_tensors_never_take_the_torch_form(gs, dev, monkeypatch):
    monkeypatch.setattr(gs.depthprior, "depth_prior_loss_torch", lambda *a, **k: pytest.fail("torch form on a HIP tensor"))
    acc, al, pr = (torch.from_numpy(t).to(dev) for t in _inputs(1, 1, 7, 13, "depth"))
    gs.depth_prior_loss_with_grad(acc, al, pr)
    with pytest.raises(ValueError, match="is on"):
        gs.depth_prior_loss_with_grad(acc, al.cpu(), pr)


# --------------------------------------------------------------------------- #
# the training routes
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("kind", ["pearson", "l1"])
def test_train_step_routes_agree_with_a_depth_prior(gs, dev, kind):
    """the one-call route (the op on the raw sums between the compositor halves) against the autograd route (the op on the
    rendered depth map), two steps each: the bounds test_gpu_depth_grad.py uses for its route comparison"""
    from gsdeblur_amd import train_step as T
    from test_gpu_depth_grad import _model_and_camera
    sc, cfg, cam = _model_and_camera(gs, dev, use_scale_regularization=True)
    target = torch.rand(96, 128, 3, generator=torch.Generator().manual_seed(5)).to(dev)
    gt = torch.rand(96, 128, 1, generator=torch.Generator().manual_seed(6)) * 4 + 2
    gt[::3] = 0.0                                              # rows without a value
    gt = gt.to(dev)
    results = []
    saved = T.TRAIN_AUTOGRAD
    try:
        for autograd_route in (0, 1):
            T.TRAIN_AUTOGRAD = autograd_route
            model = gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev)
            assert T.one_call_route(model) == (not autograd_route)
            opts = T.make_optimizers(model)
            h = [T.train_step(model, opts, cam, target, 0.2, gt_depth=gt, depth_lambda=0.5, depth_loss=kind)
                 for _ in range(2)]
            grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
            results.append((h, grads))
    finally:
        T.TRAIN_AUTOGRAD = saved
    (h0, g0), (h1, g1) = results
    for a, b in zip(h0, h1):
        print(kind, a["loss"], b["loss"])
        assert abs(a["loss"] - b["loss"]) < 1e-6
    for k in g0:
        d = (g0[k] - g1[k]).abs().max() / (g1[k].abs().max() + 1e-30)
        print(kind, k, float(d))
        assert float(d) < 2e-5, (k, float(d))
    # the prior term is in the loss and in the gradients
    model = gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev)
    h = T.train_step(model, T.make_optimizers(model), cam, target, 0.2)
    assert h0[0]["loss"] > h["loss"] + 1e-3
    assert not torch.equal(model.means.grad, g0["means"])


def test_render_and_backward_rejects_both_depth_keywords(gs, dev):
    from test_gpu_depth_grad import _model_and_camera
    sc, cfg, cam = _model_and_camera(gs, dev)
    model = gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev)
    model.train()
    with pytest.raises(ValueError, match="not both"):
        model.render_and_backward(cam, lambda rgb: torch.zeros_like(rgb), grad_depth=lambda d, a: torch.zeros_like(d),
                                  grad_depth_sums=lambda d, a: (torch.zeros_like(d), None))
    assert model.means.grad is None


def test_batch_route_is_the_mean_of_the_single_camera_losses(gs, dev):
    from gsdeblur_amd import train_step as T
    from depth_prior_e2e import views
    W, H = 128, 96
    sc = gs.data.synthetic_scene(3000, W, H, sh_degree=3, seed=77)
    cams = views(gs, sc, W, H, 8)[:2]
    cfg = gs.SplatfactoDeblurConfig(blur_samples=0, rolling_shutter_compensation=False, gamma=1.0)
    g = torch.Generator().manual_seed(12)
    images = [torch.rand(H, W, 3, generator=g).to(dev) for _ in cams]
    priors = [(torch.rand(H, W, 1, generator=g) * 4 + 2).to(dev) for _ in cams]
    single = []
    for c, im, pr in zip(cams, images, priors):
        model = gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev, num_cameras=8)
        single.append(T.train_step(model, T.make_optimizers(model), c, im, 0.2, gt_depth=pr, depth_lambda=0.5,
                                   depth_loss="pearson")["loss"])
    model = gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev, num_cameras=8)
    h = T.train_step(model, T.make_optimizers(model), cams, images, 0.2, gt_depth=priors, depth_lambda=0.5,
                     depth_loss="pearson")
    print(single, h["loss"])
    assert abs(h["loss"] - sum(single) / 2) < 1e-6
    no_depth = gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev, num_cameras=8)
    assert h["loss"] > T.train_step(no_depth, T.make_optimizers(no_depth), cams, images, 0.2)["loss"] + 1e-3


# --------------------------------------------------------------------------- #
# end to end
# --------------------------------------------------------------------------- #
# bounds of test_a_non_metric_prior_recovers_geometry_end_to_end, from its run on the MI355X (300 steps, lambda 0.5, 3.4 s):
# held-out metric depth L1 0.6893 without a depth term; 0.5831 with the depth-space prior 0.37 * depth + 1.9 (ratio 0.846),
# 0.6146 with the disparity-space prior 2 / depth + 0.1 (ratio 0.892); held-out PSNR 21.04 dB without, 20.99 / 21.11 dB with.
# Each bound lies halfway between the measured ratio and 1.
E2E_DEPTH_L1_RATIO_MAX = {"depth": 0.923, "disparity": 0.946}  # held-out metric depth L1 with the prior term / without it


def test_a_non_metric_prior_recovers_geometry_end_to_end(gs, dev):
    """The construction of test_depth_supervision_recovers_geometry_end_to_end (tools/depth_prior_e2e.py holds it), but
    the trainer sees priors that are NOT metric — 0.37 * depth + 1.9 in depth space, 2 / depth + 0.1 in disparity space
    — through depth_loss="pearson".  Against the run without a depth term on the same schedule: the held-out METRIC depth
    L1 must come out lower, the held-out PSNR no lower than the existing test's margin."""
    from depth_prior_e2e import run
    from test_gpu_depth_grad import E2E_PSNR_DROP_MAX_DB
    t0 = time.time()
    res = run(gs, dev, steps=300, depth_lambda=0.5)
    l1_0, psnr_0 = res["none"]
    for space in ("depth", "disparity"):
        l1_p, psnr_p = res[space]
        print(f"{space}: held-out depth L1 {l1_0:.4f} without / {l1_p:.4f} with the prior term (ratio {l1_p / l1_0:.3f}); "
              f"PSNR {psnr_0:.2f} / {psnr_p:.2f} dB")
    print(f"{time.time() - t0:.1f} s")
    for space in ("depth", "disparity"):
        l1_p, psnr_p = res[space]
        assert l1_p < l1_0 and l1_p <= E2E_DEPTH_L1_RATIO_MAX[space] * l1_0, (space, l1_p, l1_0)
        assert psnr_p >= psnr_0 - E2E_PSNR_DROP_MAX_DB, (space, psnr_p, psnr_0)
