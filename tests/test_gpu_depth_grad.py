"""Differentiable rendered depth: depth_acc[s] = sum_i w_i z_i gets a gradient through the weights and the depths.

Against the float64 oracle (the depth composited as a colour with the same weights), for the SE(3) sub-pose model and
the pixel-velocity model (per-sample lists, exact rolling shutter, shared list); bit-exactness of a zero depth weight,
run-to-run determinism, and the model / training surfaces (get_outputs, render_and_backward, train_step)."""
import numpy as np
import pytest
import torch

from test_gpu_parity import grad_el_ratio

pytestmark = pytest.mark.gpu

NAMES = ["means", "log_scales", "quats", "opacity_logits", "sh", "viewmat", "lin_vel", "ang_vel"]


def _scene(O, n, W, H, seed):
    sc = O.synthetic_scene(n, W, H, seed=seed, scale_mult=6.0)
    sc["lin_vel"], sc["ang_vel"] = sc["lin_vel"] * 20, sc["ang_vel"] * 10
    return sc


def _oracle_depth(O, cfg, parts, pv=None):
    """per-sample depth sums [S,H,W] from the oracle's parts: each part's pr.depths re-composited as a colour with the
    part's own list, band and row shift (float64 autograd), plus the fragile pixels of those passes.  pv: the pixel
    velocity [N,2] (times the visibility mask) of the pixel-velocity frames' row shift (_oracle_pv)"""
    S, H, W = max(1, cfg.blur_samples), cfg.img_height, cfg.img_width
    up = int(cfg.upstream_grads) & (O.UP_FOV_CLAMP | O.UP_ALPHA_CLAMP)
    pixvel = cfg.motion_model == "pixel_velocity"
    exact = pixvel and bool(cfg.rs_exact)
    n_bands = 1 if (exact or (pixvel and cfg.shared_list)) else cfg.rs_bands
    times, samp, band = O.subpose_times(cfg.blur_samples, cfg.exposure_time, n_bands, cfg.rolling_shutter_time)
    rows = O.band_tile_rows(H, n_bands)
    dt = torch.float64
    tau_rows = ((torch.arange(H, dtype=dt) + 0.5) / H - 0.5) * cfg.rolling_shutter_time if exact else None
    out = [torch.zeros(H, W, dtype=dt) for _ in range(S)]
    frag = torch.zeros(H, W, dtype=torch.bool)
    f32t = [float(np.float32(t)) for t in times]
    for p, (pr, keys, gids, bins, r, rgb, op) in enumerate(parts):
        kw = {}
        if pixvel and cfg.shared_list:
            t_c = 0.5 * (min(f32t) + max(f32t))
            row_tau = tau_rows if exact else torch.zeros(H, dtype=dt)
            kw["row_shift"] = (pv, row_tau + float(np.float32(f32t[p] - t_c)))
            s = p
        else:
            if exact:
                kw["row_shift"] = (pv, tau_rows)
            else:
                kw["tile_rows"] = rows[band[p]]
            s = samp[p]
        rd = O.rasterize_sorted(pr.xys, pr.conics, pr.depths[:, None].repeat(1, 3), op, gids, bins, H, W, None,
                                upstream=up, **kw)
        out[s] = out[s] + rd.img[..., 0]
        frag |= rd.fragile
    return torch.stack(out), frag


def _oracle_pv(O, cfg, q):
    pr0 = O.project_gaussians(q["means"], q["log_scales"].exp(), cfg.glob_scale, q["quats"], q["viewmat"], cfg.fx, cfg.fy,
                              cfg.cx, cfg.cy, cfg.img_height, cfg.img_width, O.TILE, cfg.clip_thresh, keep_offscreen=True,
                              upstream=int(cfg.upstream_grads) & O.UP_FOV_CLAMP)
    pv = O.pixel_velocity(q["means"], q["viewmat"], cfg.fx, cfg.fy, q["lin_vel"], q["ang_vel"], cfg.clip_thresh,
                          cfg.img_width, cfg.img_height, upstream=int(cfg.upstream_grads) & O.UP_FOV_CLAMP)
    return pv * (pr0.radii > 0).to(torch.float64)[:, None]


def _run_lib(gs, dev, sc, S, R, H, W, model, combined, gamma, rs_time, shared, band_rt):
    """-> (grads {name: tensor}, rgb/samples, depth_acc) of the library for loss = wd . depth_acc [+ wc . colour]"""
    et = 1 / 60
    p = {k: sc[k].to(dev).requires_grad_(True) for k in NAMES}
    if model == "se3":
        times, _, _ = gs.subpose_schedule(S, et, R, 1 / 30)
        vms = gs.subpose_viewmats(p["viewmat"], p["lin_vel"], p["ang_vel"], torch.tensor(times, device=dev))
        kw = {}
    else:
        times, _, _ = gs.subpose_schedule(S, et, R, band_rt)
        vms = p["viewmat"]
        kw = dict(lin_vel=p["lin_vel"], ang_vel=p["ang_vel"],
                  times=list(times) if shared else torch.tensor(times, device=dev, dtype=torch.float32),
                  rolling_shutter_time=rs_time, shared_list=shared)
    args = (p["means"], p["log_scales"].exp(), p["quats"], torch.sigmoid(p["opacity_logits"]), p["sh"], vms, None, S, R,
            sc["fx"], sc["fy"], sc["cx"], sc["cy"], H, W)
    if combined:
        col, _, _, dacc = gs.render_combined(*args, gamma=gamma, min_rgb_level=10.0, return_depth=True, **kw)
    else:
        col, _, _, dacc = gs.render_subposes(*args, return_depth=True, **kw)
    return p, col, dacc


def _compare(O, gs, dev, sc, cfg, S, R, model, combined, gamma, rs_time, shared, loss_kind, seed):
    H, W = cfg.img_height, cfg.img_width
    band_rt = cfg.rolling_shutter_time if R > 1 else 0.0
    p, col, dacc = _run_lib(gs, dev, sc, S, R, H, W, model, combined, gamma, rs_time, shared, band_rt)
    q = {k: sc[k].double().requires_grad_(True) for k in NAMES}
    pv = _oracle_pv(O, cfg, q) if model != "se3" else None
    out, _, samples, frag, parts, _ = O.render(cfg, q["means"], q["log_scales"].exp(), q["quats"],
                                               torch.sigmoid(q["opacity_logits"]), q["sh"], q["viewmat"], q["lin_vel"],
                                               q["ang_vel"], return_parts=True)
    dref, dfrag = _oracle_depth(O, cfg, parts, pv)
    frag = frag | dfrag
    good = ~frag
    err = (dacc.detach().cpu().double() - dref.detach())[:, good].abs().max().item()
    assert err < 2e-4 * dref.detach().max().item(), err
    wd = torch.rand(dref.shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) - 0.5
    wd[:, frag] = 0.0
    wd = wd / (H * W)
    loss_ref = (wd * dref).sum()
    loss_lib = (wd.float().to(dev) * dacc).sum()
    if loss_kind == "rgb+depth":
        cref = out if combined else samples
        wc = torch.rand(cref.shape, generator=torch.Generator().manual_seed(seed + 1), dtype=torch.float64) - 0.5
        wc[..., frag, :] = 0.0
        wc = wc * (2.0 / (H * W))
        loss_ref = loss_ref + (wc * cref).sum()
        loss_lib = loss_lib + (wc.float().to(dev) * col).sum()
    loss_ref.backward()
    loss_lib.backward()
    torch.cuda.synchronize()
    names = ["means", "log_scales", "quats", "opacity_logits", "sh", "viewmat", "lin_vel", "ang_vel"]
    if loss_kind == "depth":
        names = ["means", "log_scales", "quats", "opacity_logits", "viewmat", "lin_vel", "ang_vel"]
    ratios = {}
    for k in names:
        ref = q[k].grad
        got = p[k].grad.cpu()
        if k == "viewmat":                  # the bottom row of a rigid transform is a constant (as test_gpu_parity)
            ref, got = ref[:3], got[:3]
        if ref is None or float(ref.abs().max()) == 0.0:
            # (one blur sample: the velocities have no effect at all)
            assert float(got.abs().max()) == 0.0, k
            continue
        ratios[k] = grad_el_ratio(got.numpy(), ref.numpy())
    print("grad_el_ratio", ratios)
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("S,R,base,combined", [(1, 1, 0, False), (3, 2, 8, False), (5, 1, 0, True)])
@pytest.mark.parametrize("loss_kind", ["depth", "rgb+depth"])
def test_se3_depth_gradient_matches_oracle(gs, oracle, dev, S, R, base, combined, loss_kind):
    from gsdeblur_amd import ops
    O = oracle
    W, H, n = 128, 96, 3000
    sc = _scene(O, n, W, H, 41)
    gamma = 2.2 if combined else 1.0
    cfg = O.RenderConfig(H, W, sc["fx"], sc["fy"], sc["cx"], sc["cy"], blur_samples=S, rs_bands=R, exposure_time=1 / 60,
                         rolling_shutter_time=1 / 30, gamma=gamma, min_rgb_level=10.0 if combined else 0.0)
    old = ops.SLICE_BASE
    try:
        if base:
            ops.SLICE_BASE = base
        _compare(O, gs, dev, sc, cfg, S, R, "se3", combined, gamma, 0.0, False, loss_kind, 7)
        if base:
            assert sum(1 for x in ops.last_slice_intersects if x > 0) >= 2
    finally:
        ops.SLICE_BASE = old


@pytest.mark.parametrize("case", ["per_sample_R1", "per_sample_R2", "exact_rs", "shared"])
@pytest.mark.parametrize("loss_kind", ["depth", "rgb+depth"])
def test_pixel_velocity_depth_gradient_matches_oracle(gs, oracle, dev, case, loss_kind):
    O = oracle
    W, H, n, S = 128, 96, 3000, 3
    sc = _scene(O, n, W, H, 43)
    R = 2 if case == "per_sample_R2" else 1
    rs_time = 1 / 30 if case in ("exact_rs", "shared") else 0.0
    shared = case == "shared"
    cfg = O.RenderConfig(H, W, sc["fx"], sc["fy"], sc["cx"], sc["cy"], blur_samples=S, rs_bands=1, exposure_time=1 / 60,
                         rolling_shutter_time=rs_time, motion_model="pixel_velocity", rs_exact=rs_time != 0.0,
                         shared_list=shared)
    if R == 2:
        # per-sample lists with two rolling-shutter bands per blur sample (the band form of the readout)
        cfg = O.RenderConfig(H, W, sc["fx"], sc["fy"], sc["cx"], sc["cy"], blur_samples=S, rs_bands=R,
                             exposure_time=1 / 60, rolling_shutter_time=1 / 30, motion_model="pixel_velocity")
    _compare(O, gs, dev, sc, cfg, S, R, "pixvel", False, 1.0, rs_time, shared, loss_kind, 11)


def test_exact_rolling_shutter_depth_gradient_in_one_slice_matches_oracle(gs, oracle, dev):
    """the cases above are frames of several depth slices; one of 4 x 3 tiles and 400 Gaussians fits into one, so the exact
    rolling-shutter backward runs without reverse-traversal state (raster_bwd_rs_kernel<false, true>)"""
    from gsdeblur_amd import ops
    O = oracle
    W, H, n, S = 64, 48, 400, 2
    sc = _scene(O, n, W, H, 43)
    cfg = O.RenderConfig(H, W, sc["fx"], sc["fy"], sc["cx"], sc["cy"], blur_samples=S, rs_bands=1, exposure_time=1 / 60,
                         rolling_shutter_time=1 / 30, motion_model="pixel_velocity", rs_exact=True, shared_list=False)
    _compare(O, gs, dev, sc, cfg, S, 1, "pixvel", False, 1.0, 1 / 30, False, "rgb+depth", 11)
    assert sum(1 for x in ops.last_slice_intersects if x > 0) == 1


def _frame_grads(gs, dev, sc, v_depth_scale, motion="se3", seed=3):
    """render_step of one frame with an rgb gradient and (v_depth_scale not None) a depth gradient; -> grads dict"""
    from gsdeblur_amd.step import render_step
    W, H, S = sc["W"], sc["H"], 3
    times = torch.tensor(gs.subpose_schedule(S, 1 / 60, 1, 0.0)[0], device=dev, dtype=torch.float32)
    g_img = (torch.rand(H, W, 3, generator=torch.Generator().manual_seed(seed)) - 0.5).to(dev)
    gd = None
    if v_depth_scale is not None:
        gd = ((torch.rand(S, H, W, generator=torch.Generator().manual_seed(seed + 1)) - 0.5) * v_depth_scale).to(dev)
    p = {k: sc[k].to(dev) for k in NAMES}
    _, g, _ = render_step(p["means"], p["log_scales"], p["quats"], p["opacity_logits"], p["sh"], p["viewmat"],
                          p["lin_vel"], p["ang_vel"], times, None, S, 1, sc["fx"], sc["fy"], sc["cx"], sc["cy"], H, W,
                          g_img, gamma=2.2, min_rgb_level=10.0, raw_params=True, motion_model=motion, grad_depth=gd)
    torch.cuda.synchronize()
    return {k: (v.clone() if v is not None else None) for k, v in g.items()}


@pytest.mark.parametrize("motion", ["se3", "pixel_velocity"])
def test_zero_depth_weight_is_bit_identical_to_rgb_only(gs, oracle, dev, motion):
    sc = _scene(oracle, 20000, 192, 128, 5)
    sc["W"], sc["H"] = 192, 128
    a = _frame_grads(gs, dev, sc, None, motion)
    b = _frame_grads(gs, dev, sc, 0.0, motion)          # v_depth = zeros: the depth kernels run
    for k in ("means", "scales", "quats", "opacities", "sh", "viewmat", "lin_vel", "ang_vel"):
        assert a[k] is not None and torch.equal(a[k], b[k]), k


def test_depth_gradient_is_deterministic(gs, oracle, dev):
    sc = _scene(oracle, 20000, 192, 128, 6)
    sc["W"], sc["H"] = 192, 128
    a = _frame_grads(gs, dev, sc, 1.0)
    b = _frame_grads(gs, dev, sc, 1.0)
    for k in ("viewmat", "lin_vel", "ang_vel"):
        assert torch.equal(a[k], b[k]), k
    c = _frame_grads(gs, dev, sc, None)
    assert not torch.equal(a["means"], c["means"])      # the depth term arrived


def _model_and_camera(gs, dev, n=6000, W=128, H=96, seed=31, **cfg_kw):
    sc = gs.data.synthetic_scene(n, W, H, sh_degree=3, seed=seed)
    sc["lin_vel"], sc["ang_vel"] = sc["lin_vel"] * 20, sc["ang_vel"] * 10
    c2w = torch.eye(4)[:3].clone()
    c2w[:, 1] *= -1
    c2w[:, 2] *= -1
    flip = torch.tensor([1.0, -1.0, -1.0])
    cam = gs.Camera(c2w, sc["fx"], sc["fy"], sc["cx"], sc["cy"], W, H,
                    metadata=dict(cam_idx=0, camera_linear_velocity=[float(v) for v in sc["lin_vel"] * flip],
                                  camera_angular_velocity=[float(v) for v in sc["ang_vel"] * flip],
                                  exposure_time=1 / 60, rolling_shutter_time=0.0))
    cfg = gs.SplatfactoDeblurConfig(blur_samples=3, rolling_shutter_compensation=False, gamma=2.2, min_rgb_level=10.0,
                                    background_color="auto", **cfg_kw)
    cfg.camera_optimizer.mode = "SO3xR3"
    cfg.camera_velocity_optimizer.enabled = True
    return sc, cfg, cam


def test_model_depth_output_is_differentiable(gs, dev):
    sc, cfg, cam = _model_and_camera(gs, dev, output_depth_during_training=True)
    model = gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev)
    model.train()
    out = model.get_outputs(cam)
    assert out["depth"].requires_grad
    out["depth"][out["accumulation"] > 0.5].mean().backward()
    assert float(model.means.grad.abs().max()) > 0
    assert float(model.pose_adjustment.grad.abs().max()) > 0


def test_render_and_backward_depth_matches_autograd(gs, dev):
    sc, cfg, cam = _model_and_camera(gs, dev)
    gt = (torch.rand(96, 128, 1, generator=torch.Generator().manual_seed(2)) * 4 + 2).to(dev)
    res = []
    for route in (0, 1):
        model = gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev)
        model.train()
        if route == 0:
            def grad_depth(depth, acc):
                return torch.sign(depth - gt) * (acc > 0) / gt.numel()
            model.render_and_backward(cam, lambda rgb: torch.full_like(rgb, 1e-3), grad_depth)
        else:
            out = model.get_outputs(cam, return_depth=True)
            loss = (out["rgb"] * 1e-3).sum() + (torch.abs(out["depth"] - gt) * (out["accumulation"] > 0)).sum() / gt.numel()
            loss.backward()
        res.append({k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})
    for k in res[0]:
        assert float(res[0][k].abs().max()) > 0, k
        d = (res[0][k] - res[1][k]).abs().max() / (res[1][k].abs().max() + 1e-30)
        assert float(d) < 2e-5, (k, float(d))


def test_train_step_with_depth_routes_agree(gs, dev):
    from gsdeblur_amd import train_step as T
    sc, cfg, cam = _model_and_camera(gs, dev, use_scale_regularization=True)
    target = torch.rand(96, 128, 3, generator=torch.Generator().manual_seed(5)).to(dev)
    gt = torch.rand(96, 128, 1, generator=torch.Generator().manual_seed(6)) * 4 + 2
    gt[::3] = 0.0                                              # rows without a measurement
    gt = gt.to(dev)
    results = []
    saved = T.TRAIN_AUTOGRAD
    try:
        for autograd_route in (0, 1):
            T.TRAIN_AUTOGRAD = autograd_route
            model = gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev)
            assert T.one_call_route(model) == (not autograd_route)
            opts = T.make_optimizers(model)
            h = [T.train_step(model, opts, cam, target, 0.2, gt_depth=gt, depth_lambda=0.5) for _ in range(2)]
            grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
            results.append((h, grads))
    finally:
        T.TRAIN_AUTOGRAD = saved
    (h0, g0), (h1, g1) = results
    for a, b in zip(h0, h1):
        assert abs(a["loss"] - b["loss"]) < 1e-6
    for k in g0:
        d = (g0[k] - g1[k]).abs().max() / (g1[k].abs().max() + 1e-30)
        assert float(d) < 2e-5, (k, float(d))
    # the depth term is in the loss: without it the loss is smaller by about lambda * L1
    model = gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev)
    h = T.train_step(model, T.make_optimizers(model), cam, target, 0.2)
    assert h0[0]["loss"] > h["loss"] + 1e-3


def test_twin_backend_raises_on_depth_gradient(gs, oracle, dev, monkeypatch):
    from gsdeblur_amd import ops
    monkeypatch.setattr(ops, "NATIVE_FRAME", 0)
    sc = _scene(oracle, 2000, 96, 64, 8)
    p = {k: sc[k].to(dev).requires_grad_(True) for k in NAMES}
    vms = gs.subpose_viewmats(p["viewmat"], p["lin_vel"], p["ang_vel"], torch.tensor([0.0], device=dev))
    _, _, _, dacc = gs.render_subposes(p["means"], p["log_scales"].exp(), p["quats"], torch.sigmoid(p["opacity_logits"]),
                                       p["sh"], vms, None, 1, 1, sc["fx"], sc["fy"], sc["cx"], sc["cy"], 64, 96,
                                       return_depth=True)
    with pytest.raises(NotImplementedError):
        dacc.sum().backward()


def _views(gs, sc, W, H, n_views):
    """n_views pinhole cameras around the scene's own (OpenGL camera-to-world, no motion): a small orbit of positions"""
    import math
    cams = []
    for v in range(n_views):
        c2w = torch.eye(4)[:3].clone()
        c2w[:, 1] *= -1
        c2w[:, 2] *= -1
        ph = 2.0 * math.pi * v / n_views
        c2w[:, 3] = torch.tensor([0.25 * math.cos(ph), 0.15 * math.sin(ph), 0.0])
        cams.append(gs.Camera(c2w, sc["fx"], sc["fy"], sc["cx"], sc["cy"], W, H,
                              metadata=dict(cam_idx=v, camera_linear_velocity=[0.0, 0.0, 0.0],
                                            camera_angular_velocity=[0.0, 0.0, 0.0], exposure_time=0.0,
                                            rolling_shutter_time=0.0)))
    return cams


def _held_out_depth_l1(model, cams, depths, idx):
    errs = []
    for i in idx:
        out = model.get_outputs_for_camera(cams[i])
        valid = depths[i] > 0
        errs.append(float((out["depth"] - depths[i]).abs()[valid].mean()))
    return sum(errs) / len(errs)


# bounds of test_depth_supervision_recovers_geometry_end_to_end, from its run on the MI355X: held-out depth L1 0.689
# without / 0.436 with the depth term (ratio 0.633), held-out PSNR 21.04 / 21.02 dB (drop 0.02 dB), 5.2 s
E2E_DEPTH_L1_RATIO_MAX = 0.75      # held-out depth L1 with the depth term / without it
E2E_PSNR_DROP_MAX_DB = 0.3         # held-out PSNR without the depth term minus PSNR with it


def test_depth_supervision_recovers_geometry_end_to_end(gs, dev):
    """Seeded synthetic scene; ground-truth rgb and depth rendered by the library from 8 views; the model starts from the
    same Gaussians with their means pushed along the rays of the central camera (scales pushed with them, so the first
    views barely change).  Trained with depth_lambda > 0 and with depth_lambda = 0 on the SAME schedule: the held-out
    depth error must come out clearly lower with the depth term, the held-out PSNR no lower than a stated margin."""
    import types
    import time
    from gsdeblur_amd import training as T
    t0 = time.time()
    n, W, H = 3000, 128, 96
    sc = gs.data.synthetic_scene(n, W, H, sh_degree=3, seed=77)
    cams = _views(gs, sc, W, H, 8)
    cfg = gs.SplatfactoDeblurConfig(blur_samples=0, rolling_shutter_compensation=False, gamma=1.0)
    gt_model = gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev)
    images, depths = [], []
    with torch.no_grad():
        for c in cams:
            out = gt_model.get_outputs_for_camera(c)
            images.append(out["rgb"].clamp(0, 1).contiguous())
            depths.append(torch.where(out["accumulation"] > 0.5, out["depth"], torch.zeros_like(out["depth"])).contiguous())
    g = torch.Generator().manual_seed(78)
    push = (torch.rand(n, 1, generator=g) * 0.3 + 0.15) * torch.where(torch.rand(n, 1, generator=g) < 0.5, -1.0, 1.0)
    start = dict(sc)
    start["means"] = sc["means"] * (1.0 + push)                       # along the ray through the camera centre (0, 0, 0)
    start["log_scales"] = sc["log_scales"] + torch.log1p(push)
    scene = types.SimpleNamespace(cameras=cams, train_indices=[1, 2, 3, 5, 6, 7], eval_indices=[0, 4])
    res = {}
    for lam in (0.0, 0.5):
        model = gs.SplatfactoDeblurModel.from_scene(cfg, start, dev)
        torch.manual_seed(0)
        r = T.train_scene(model, scene, images, 300, depths=depths, depth_lambda=lam, seed=3)
        res[lam] = (_held_out_depth_l1(model, cams, depths, scene.eval_indices), r["results"]["psnr"])
    l1_0, psnr_0 = res[0.0]
    l1_d, psnr_d = res[0.5]
    print(f"held-out depth L1: {l1_0:.4f} without / {l1_d:.4f} with the depth term (ratio {l1_d / l1_0:.3f}); "
          f"PSNR {psnr_0:.2f} / {psnr_d:.2f} dB; {time.time() - t0:.1f} s")
    assert l1_d <= E2E_DEPTH_L1_RATIO_MAX * l1_0, (l1_d, l1_0)
    assert psnr_d >= psnr_0 - E2E_PSNR_DROP_MAX_DB, (psnr_d, psnr_0)
    assert time.time() - t0 < 60.0


def test_full_size_rgb_plus_depth_step(gs, dev):
    """The bench's headline scene (1M Gaussians, 1920x1080, S = 5 sub-poses) through render_step with an rgb and a depth
    gradient: finite gradients, the depth term arrives; a zero depth weight gives the rgb-only step's gradients bit for
    bit.  Once as the headline runs (one depth slice), once with a small slice budget (several slices: the backward's
    reverse-traversal state carries the depth term between them)."""
    import bench
    from gsdeblur_amd import ops
    wl = bench.Workload(gs, dev, 0, 1, 1_000_000, 1920, 1080, 5, 1, "survey", "sparse")
    p, sc = wl.params, wl.sc
    S, H, W = 5, 1080, 1920
    keys = ("means", "scales", "quats", "opacities", "sh", "viewmat", "lin_vel", "ang_vel")

    def step(grad_depth):
        _, g, _ = gs.render_step(p["means"], p["log_scales"], p["quats"], p["opacity_logits"], p["sh"], wl.viewmat,
                                 wl.lin, wl.ang, wl.times_t, wl.bg, S, 1, sc["fx"], sc["fy"], sc["cx"], sc["cy"], H, W,
                                 wl.wt, gamma=2.2, min_rgb_level=10.0, raw_params=True, hints=wl.hints,
                                 grad_depth=grad_depth)
        torch.cuda.synchronize()
        return {k: g[k].clone() for k in keys}

    v_depth = ((torch.rand(S, H, W, generator=torch.Generator().manual_seed(9)) - 0.5) * 1e-2).to(dev)
    saved = ops.SLICE_BASE
    try:
        for base in (None, 16):
            if base is not None:
                ops.SLICE_BASE = base
                wl.hints = ops.FrameHints()
            for _ in range(3):
                step(None)                             # settle the frame hints (slice budget, arena)
            rgb = step(None)
            if base is not None:
                assert sum(1 for x in ops.last_slice_intersects if x > 0) >= 2
            both = step(v_depth)
            zero = step(torch.zeros_like(v_depth))
            for k in keys:
                assert torch.isfinite(both[k]).all(), k
                assert torch.equal(zero[k], rgb[k]), k
            assert not torch.equal(both["means"], rgb["means"]) and not torch.equal(both["viewmat"], rgb["viewmat"])
    finally:
        ops.SLICE_BASE = saved
