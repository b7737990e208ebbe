"""The depth-derived normals and their two losses on the MI355X: the kernels of csrc/normals.hip against the float64
reference (tests/normal_reference.py, whose docstring states the tolerance rule), bit-identity, the autograd form, the
training routes, and whether normal priors recover surface orientation end to end."""
import functools
import time

import numpy as np
import pytest
import torch

import normal_reference as R
from test_normals_host import GROUP, K_THREADS, MANY_GROUPS, SIZES, TH, TW, term_args

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=4)
def _inputs(B, S, H, W):
    """the inputs of a shape, made once and shared by its cases (never written)"""
    batch = R.make_batch(B, S, H, W, seed=11 + H + W)
    for b in range(B):
        R.assert_input_conditions(batch[0][b], batch[1][b], batch[2][b], batch[3][b])
    return batch


def _run(gs, dev, acc, al, K, prior=None, guide=None, **kw):
    f = lambda t: None if t is None else torch.from_numpy(np.ascontiguousarray(t)).to(dev)   # noqa: E731
    out = gs.normal_loss_with_grad(f(acc), f(al), torch.from_numpy(K), f(prior), f(guide), return_stats=True,
                                   return_normals=True, **kw)
    return tuple(t.cpu().numpy() for t in out)


def test_sizes_cover_what_they_claim():
    assert {w for h, w in SIZES if h == TH + 1} >= {TW - 1, TW, TW + 1, 2 * TW + 1, GROUP * TW + 1}
    assert {h for h, w in SIZES if w == TW + 1} >= {TH - 1, TH, TH + 1, 2 * TH + 1}
    assert -(-MANY_GROUPS[1] // (TW * GROUP)) * -(-MANY_GROUPS[0] // TH) > K_THREADS     # the record loop takes a second trip


@pytest.mark.parametrize("term", list(R.TERMS))           # varies fastest: the terms of a shape share its inputs
@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("size", SIZES + [MANY_GROUPS], ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernels_match_the_reference(gs, dev, term, S, B, size):
    """loss, both gradients and the normals against the reference under the project's rule (4 x what float32 storage costs
    the reference itself + 1e-6; gradients and normals relative to the frame's largest reference value); counts exact;
    exact zeros at every pixel without z and for the degenerate frames of the B = 3 batch (no prior value at all, which
    leaves only the smoothness term, and alpha 0 everywhere); every frame of a batch bit-identical to that frame alone"""
    H, W = size
    acc, al, K, prior, guide = _inputs(B, S, H, W)
    pr, gd, kw = term_args(term, prior, guide)
    loss, vd, va, stats, n = _run(gs, dev, acc, al, K, pr, gd, **kw)
    assert loss.shape == (B,) and vd.shape == acc.shape and va.shape == al.shape and stats.shape == (B, 6)
    assert n.shape == (B, H, W, 3)
    for b in range(B):
        pb, gb = (None if pr is None else pr[b]), (None if gd is None else gd[b])
        fig = R.check_frame(loss[b], vd[b], va[b], n[b], stats[b], acc[b], al[b], K[b], what=(term, S, b, size), prior=pb,
                            guide=gb, **kw)
        if b == 0 and H >= 4 and W >= 4:
            assert vd[b].any() and va[b].any()
        if B == 3 and (b == 2 or (b == 1 and term == "prior")):
            assert loss[b] == 0 and not vd[b].any() and not va[b].any()
        if B > 1:
            l1, vd1, va1, st1, n1 = _run(gs, dev, acc[b], al[b], K[b], pb, gb, **kw)
            assert l1 == loss[b] and np.array_equal(vd1, vd[b]) and np.array_equal(va1, va[b])
            assert np.array_equal(st1, stats[b]) and np.array_equal(n1, n[b])
    print(fig)


def test_depth_normals_alone_gives_the_loss_call_its_normals(gs, dev):
    for size in ((67, 131), (TH + 1, GROUP * TW + 1)):
        acc, al, K, prior, _ = _inputs(3, 5, *size)
        n = _run(gs, dev, acc, al, K, prior)[4]
        alone = gs.depth_normals(torch.from_numpy(acc).to(dev), torch.from_numpy(al).to(dev), torch.from_numpy(K))
        assert np.array_equal(alone.cpu().numpy(), n) and n.any()
        one = gs.depth_normals(torch.from_numpy(acc[0]).to(dev), torch.from_numpy(al[0]).to(dev), tuple(K[0].tolist()))
        assert one.shape == size + (3,) and np.array_equal(one.cpu().numpy(), n[0])


def test_min_alpha_leaves_pixels_out(gs, dev):
    acc, al, K, prior, guide = R.make_frame(5, 67, 131, seed=9)
    al = al.copy()
    al[:, 5] *= 0.01
    kw = dict(prior_weight=0.7, smooth_weight=0.4, edge_beta=2.0, min_alpha=0.02)
    loss, vd, va, stats, n = _run(gs, dev, acc, al, K, prior, guide, **kw)
    R.check_frame(loss, vd, va, n, stats, acc, al, K, prior=prior, guide=guide, **kw)
    assert not vd[:, 5].any() and not n[4:7].any() and vd[:, 7].any() and n[7].any()


def test_two_runs_and_a_full_size_call_agree_bit_for_bit(gs, dev):
    """1080p, S = 5, both terms: finite and non-zero, two runs of the same call give the same bits; a strip of alpha 0 has
    zero gradient and non-zero gradient next to it"""
    S, H, W = 5, 1080, 1920
    g = torch.Generator().manual_seed(4)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    depth = 4.0 + 0.8 * torch.sin(x / 9.0) + 0.5 * torch.cos(y / 7.0) + 0.05 * torch.randn(H, W, generator=g)
    al = torch.rand(S, H, W, generator=g) * 0.9 + 0.1
    al[:, :, 64:128] = 0.0
    acc, al = (al * depth).to(dev), al.to(dev)
    prior = torch.randn(H, W, 3, generator=g) * 0.3 + torch.tensor([0.0, 0.0, -1.0])
    prior, guide = prior.to(dev), torch.rand(H, W, 3, generator=g).to(dev)
    K = (0.9 * W, 0.9 * W, 0.5 * W, 0.5 * H)
    kw = dict(prior_weight=0.3, smooth_weight=0.2, edge_beta=2.0, return_stats=True, return_normals=True)
    one = gs.normal_loss_with_grad(acc, al, K, prior, guide, **kw)
    two = gs.normal_loss_with_grad(acc, al, K, prior, guide, **kw)
    for a, b in zip(one, two):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    loss, vd, va, stats, n = one
    assert float(loss) > 0 and float(stats[0]) == (H - 2) * ((63 - 1) + (W - 1 - 129))
    assert not vd[:, :, 64:128].any() and not va[:, :, 64:128].any() and not n[:, 63:129].any()
    assert vd[:, 1:-1, 63].all() and vd[:, 1:-1, 128].all() and va[:, 1:-1, 128].all() and vd[:, :, 200:].any()


def test_autograd_form_and_upstream_gradient(gs, dev):
    acc, al, K, prior, guide = _inputs(3, 5, 67, 131)
    acc, al, prior, guide = (torch.from_numpy(t).to(dev) for t in (acc, al, prior, guide))
    K = torch.from_numpy(K)
    kw = dict(prior_weight=0.7, smooth_weight=0.4, edge_beta=2.0)
    loss, vd, va = gs.normal_loss_with_grad(acc, al, K, prior, guide, **kw)
    a, b = acc.clone().requires_grad_(True), al.clone().requires_grad_(True)
    out = gs.normal_loss(a, b, K, prior, guide, **kw)
    assert torch.equal(out.detach(), loss)
    out.sum().backward()
    assert torch.equal(a.grad, vd) and torch.equal(b.grad, va)
    a.grad = b.grad = None
    (gs.normal_loss(a, b, K, prior, guide, **kw) * 0.5).sum().backward()
    assert torch.equal(a.grad, vd * 0.5) and torch.equal(b.grad, va * 0.5)
    a1 = acc[0].clone().requires_grad_(True)
    s = gs.normal_loss(a1, al[0], K[0], prior[0], guide[0], **kw)
    assert s.shape == () and torch.equal(s.detach(), loss[0])
    s.backward()
    assert torch.equal(a1.grad, vd[0])


def test_hip_tensors_never_take_the_torch_form(gs, dev, monkeypatch):
    monkeypatch.setattr(gs.normals, "normal_loss_torch", lambda *a, **k: pytest.fail("torch form on a HIP tensor"))
    monkeypatch.setattr(gs.normals, "depth_normals_torch", lambda *a, **k: pytest.fail("torch form on a HIP tensor"))
    acc, al, K, prior, _ = _inputs(1, 1, 7, 13)
    acc, al, prior = (torch.from_numpy(t).to(dev) for t in (acc, al, prior))
    gs.normal_loss_with_grad(acc, al, K, prior)
    gs.depth_normals(acc, al, K)
    with pytest.raises(ValueError, match="is on"):
        gs.normal_loss_with_grad(acc, al.cpu(), K, prior)
    with pytest.raises(ValueError, match="is on"):
        gs.normal_loss_with_grad(acc, al, K, prior.cpu())


# --------------------------------------------------------------------------- #
# the training routes
# --------------------------------------------------------------------------- #
def _training_inputs(dev):
    target = torch.rand(96, 128, 3, generator=torch.Generator().manual_seed(5)).to(dev)
    g = torch.Generator().manual_seed(6)
    prior = torch.randn(96, 128, 3, generator=g) * 0.3 + torch.tensor([0.0, 0.0, -1.0])
    prior[::3] = 0.0                                           # rows without a value
    gt = torch.rand(96, 128, 1, generator=g) * 4 + 2
    return target, prior.to(dev), gt.to(dev)


NORMAL_KW = dict(normal_lambda=0.5, normal_smooth_lambda=0.3, normal_edge_beta=2.0)


@pytest.mark.parametrize("with_depth", [False, "pearson", "metric"], ids=["normals", "normals+pearson", "normals+metric"])
def test_train_step_routes_agree_with_a_normal_prior(gs, dev, with_depth):
    """the one-call route (the op on the raw sums between the compositor halves) against the autograd route (the op on the
    rendered depth map), two steps each, with a normal prior plus smoothness, alone, together with the Pearson depth
    prior and together with the metric depth L1 (whose chain then runs on the sums too): the bounds of
    test_gpu_depthprior.py's route comparison"""
    from gsdeblur_amd import train_step as T
    from test_gpu_depth_grad import _model_and_camera
    sc, cfg, cam = _model_and_camera(gs, dev, use_scale_regularization=True)
    target, prior, gt = _training_inputs(dev)
    kw = dict(NORMAL_KW, gt_normal=prior)
    if with_depth:
        kw.update(gt_depth=gt, depth_lambda=0.5, depth_loss=None if with_depth == "metric" else with_depth)
    results = []
    saved = T.TRAIN_AUTOGRAD
    try:
        for autograd_route in (0, 1):
            T.TRAIN_AUTOGRAD = autograd_route
            model = gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev)
            assert T.one_call_route(model) == (not autograd_route)
            opts = T.make_optimizers(model)
            h = [T.train_step(model, opts, cam, target, 0.2, **kw) for _ in range(2)]
            grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
            results.append((h, grads))
    finally:
        T.TRAIN_AUTOGRAD = saved
    (h0, g0), (h1, g1) = results
    worst = {}
    for a, b in zip(h0, h1):
        print(with_depth, a["loss"], b["loss"])
        worst["loss"] = max(worst.get("loss", 0.0), abs(a["loss"] - b["loss"]))
    for k in g0:
        worst[k] = float((g0[k] - g1[k]).abs().max() / (g1[k].abs().max() + 1e-30))
    print(with_depth, worst)
    assert worst.pop("loss") < 1e-6
    for k, d in worst.items():
        assert d < 2e-5, (k, d)
    # the term is in the loss and in the gradients
    model = gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev)
    h = T.train_step(model, T.make_optimizers(model), cam, target, 0.2)
    assert h0[0]["loss"] > h["loss"] + 1e-3
    assert not torch.equal(model.means.grad, g0["means"])


def test_default_keywords_leave_the_step_bit_identical(gs, dev):
    from gsdeblur_amd import train_step as T
    from test_gpu_depth_grad import _model_and_camera
    sc, cfg, cam = _model_and_camera(gs, dev, use_scale_regularization=True)
    target, prior, gt = _training_inputs(dev)
    res = []
    for kw in ({}, dict(gt_normal=None, normal_lambda=0.0, normal_smooth_lambda=0.0, normal_edge_beta=0.0),
               dict(gt_normal=prior, normal_lambda=0.0, normal_edge_beta=3.0)):
        model = gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev)
        h = T.train_step(model, T.make_optimizers(model), cam, target, 0.2, gt_depth=gt, depth_lambda=0.5, depth_loss="pearson",
                         **kw)
        res.append((h, {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}))
    for h, g in res[1:]:
        assert h == res[0][0] and g.keys() == res[0][1].keys()
        assert all(torch.equal(g[k], res[0][1][k]) for k in g)


def test_batch_route_is_the_mean_of_the_single_camera_losses(gs, dev):
    from gsdeblur_amd import train_step as T
    from depth_prior_e2e import views
    W, H = 128, 96
    sc = gs.data.synthetic_scene(3000, W, H, sh_degree=3, seed=77)
    cams = views(gs, sc, W, H, 8)[:2]
    cfg = gs.SplatfactoDeblurConfig(blur_samples=0, rolling_shutter_compensation=False, gamma=1.0)
    g = torch.Generator().manual_seed(12)
    images = [torch.rand(H, W, 3, generator=g).to(dev) for _ in cams]
    priors = [(torch.randn(H, W, 3, generator=g) * 0.3 + torch.tensor([0.0, 0.0, -1.0])).to(dev) for _ in cams]
    single = []
    for c, im, pr in zip(cams, images, priors):
        model = gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev, num_cameras=8)
        single.append(T.train_step(model, T.make_optimizers(model), c, im, 0.2, gt_normal=pr, **NORMAL_KW)["loss"])
    model = gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev, num_cameras=8)
    h = T.train_step(model, T.make_optimizers(model), cams, images, 0.2, gt_normal=priors, **NORMAL_KW)
    print(single, h["loss"])
    assert abs(h["loss"] - sum(single) / 2) < 1e-6
    plain = gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev, num_cameras=8)
    assert h["loss"] > T.train_step(plain, T.make_optimizers(plain), cams, images, 0.2)["loss"] + 1e-3


def test_render_normals(gs, dev):
    from test_gpu_depth_grad import _model_and_camera
    sc, cfg, cam = _model_and_camera(gs, dev)
    model = gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev)
    n = model.render_normals(cam)
    assert n.shape == (96, 128, 3) and not n.requires_grad and model.training
    has = (n != 0).any(-1)
    assert has.sum() > 1000 and torch.allclose(n[has].norm(dim=-1), torch.ones((), device=dev), atol=1e-5)
    assert (n[has][:, 2] < 0).float().mean() > 0.5            # towards the camera
    out = model.sharp_outputs(cam)
    m = (out["accumulation"].reshape(1, 96, 128) > 0.5).float()
    want = gs.depth_normals(out["depth"].reshape(1, 96, 128) * m, m, (cam.fx, cam.fy, cam.cx, cam.cy))
    assert torch.equal(n, want)


# --------------------------------------------------------------------------- #
# end to end
# --------------------------------------------------------------------------- #
# bounds of test_normal_priors_recover_orientation_end_to_end, from its run on the MI355X (300 steps, normal_lambda 0.02): the
# held-out mean angle between the model's depth-derived normals and the true scene's is 57.32 deg without the term and
# 55.69 deg with the prior term (ratio 0.972); held-out depth L1 0.6893 / 0.6681, PSNR 21.04 / 21.13 dB.  The bound lies
# halfway between the measured ratio and 1.  At 128 x 96 with 3000 Gaussians the normals of the rendered depth are dominated
# by splat-sized roughness, so the effect is small (0.948 after 1000 steps at lambda 0.1 plus smoothness 0.05); larger weights
# make it worse (1.02 at 0.2, 1.07 at 0.5), and smoothness ALONE does not improve the angle at this size (1.005 at 0.01,
# 1.014 at 0.02, 1.022 at 0.05): DESIGN 5.15 records both as negatives, and that case is not part of the test.
E2E_KW = dict(steps=300, normal_lambda=0.02, smooth_lambda=0.01)
E2E_ANGLE_RATIO_MAX = {"prior": 0.986}                    # held-out normal angle with the term / without it


def test_normal_priors_recover_orientation_end_to_end(gs, dev):
    """The construction of tools/depth_prior_e2e.py (tools/normal_e2e.py holds this one): the trainer sees normal priors
    that are gs.depth_normals of the TRUE scene's rendered depth.  Against the run without the term on the same schedule:
    the held-out mean angle between the model's depth-derived normals and the true scene's must come out lower, the
    held-out PSNR no lower than the existing depth test's margin."""
    from normal_e2e import run
    from test_gpu_depth_grad import E2E_PSNR_DROP_MAX_DB
    t0 = time.time()
    res = run(gs, dev, variants=("none",) + tuple(E2E_ANGLE_RATIO_MAX), **E2E_KW)
    a0, l0, p0 = res["none"]
    for name in E2E_ANGLE_RATIO_MAX:
        a, l, p = res[name]
        print(f"{name}: held-out normal angle {a0:.3f} deg without / {a:.3f} deg with the term (ratio {a / a0:.3f}); "
              f"depth L1 {l0:.4f} / {l:.4f}; PSNR {p0:.2f} / {p:.2f} dB")
    print(f"{time.time() - t0:.1f} s")
    for name, bound in E2E_ANGLE_RATIO_MAX.items():
        a, l, p = res[name]
        assert a < a0 and a <= bound * a0, (name, a, a0)
        assert p >= p0 - E2E_PSNR_DROP_MAX_DB, (name, p, p0)
