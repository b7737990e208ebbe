"""Every spherical-harmonics degree on the fused frame path.

The rest of the GPU suite renders at SH degree 3 with K = 16 coefficients.  Here the frame runs at every (active degree,
allocated K) pair — K above (deg + 1)^2 is the progressive schedule — in both coefficient layouts, against the float64
oracle, on scenes whose higher bands carry signal and whose colour clamp is active (tests/sh_degree_cases.py); every
degree-4 (`<25>`) instantiation of csrc/project.hip that Python can reach is launched and checked; the model, both
optimizers, densification and the row kernels run with the zero-width features_rest of degree 0 and the 72-wide one of
degree 4."""
import ctypes
import math

import pytest
import torch

import sh_degree_cases as C
import test_gpu_parity as TP
from test_gpu_parity import IMG_ATOL, check_fragile, grad_el_ratio, images_close, rel_max
from test_gpu_depth_grad import _oracle_depth

pytestmark = pytest.mark.gpu

TP.FRAGILE_OBSERVED.update({f"{C.tag(d, k)}": v for (d, k), v in C.FRAGILE_OBSERVED.items()})
TP.FRAGILE_OBSERVED.update({f"{C.tag(d, k, 'pixvel')}": v for (d, k), v in C.FRAGILE_OBSERVED_PIXVEL.items()})

G_NAMES = ["means", "log_scales", "quats", "opacity_logits", "sh"]
H, W, S, R = C.H, C.W, C.S, C.R


def _hip_frame(gs, dev, sc, deg, layout="single", model="se3", wt=None, wd=None):
    """the library's frame of a case, two-step (per-sample images, then the averaging), loss = wt . image [+ wd . depth]
    -> (image, samples, radii, depth sums or None, gradients by oracle name; "sh" re-assembled from dc / rest)"""
    names = [k for k in C.NAMES if k != "sh"]
    p = {k: sc[k].float().to(dev).clone().requires_grad_(True) for k in names}
    sh = sc["sh"].float().to(dev)
    times, _, _ = gs.subpose_schedule(S, C.ET, R, C.RT)
    tt = torch.tensor(times, device=dev)
    if model == "se3":
        vms, kw = gs.subpose_viewmats(p["viewmat"], p["lin_vel"], p["ang_vel"], tt), {}
    else:
        vms, kw = p["viewmat"], dict(lin_vel=p["lin_vel"], ang_vel=p["ang_vel"], times=tt)
    if layout == "single":
        coef = [sh.clone().requires_grad_(True)]
        args = (p["means"], p["log_scales"].exp(), p["quats"], torch.sigmoid(p["opacity_logits"]), coef[0])
    else:
        coef = [sh[:, 0, :].clone().requires_grad_(True), sh[:, 1:, :].clone().requires_grad_(True)]
        assert coef[1].shape == (sh.shape[0], sh.shape[1] - 1, 3)
        args = (p["means"], p["log_scales"], p["quats"], p["opacity_logits"], coef[0])
        kw.update(sh_rest=coef[1], raw_params=True)
    out = gs.render_subposes(*args, vms, C.BG.to(dev), S, R, sc["fx"], sc["fy"], sc["cx"], sc["cy"], H, W, sh_degree=deg,
                             antialiased=True, return_depth=wd is not None, **kw)
    samples, radii = out[0], out[2]
    dacc = out[3] if wd is not None else None
    img = gs.combine_samples(samples, C.GAMMA, C.MLEVEL)
    loss = (img * wt.float().to(dev)).sum()
    if wd is not None:
        loss = loss + (dacc * wd.float().to(dev)).sum()
    loss.backward()
    torch.cuda.synchronize()
    g = {k: p[k].grad.detach().clone() for k in names}
    if layout == "single":
        g["sh"] = coef[0].grad.detach().clone()
    else:
        assert coef[0].grad.shape == coef[0].shape and coef[1].grad.shape == coef[1].shape
        g["sh"] = torch.cat([coef[0].grad[:, None, :], coef[1].grad], dim=1)
    return img.detach(), samples.detach(), radii, (None if dacc is None else dacc.detach()), g


def _check_unused_bands_and_rows(g, radii, nb, what):
    """bands the active degree does not use get EXACT zeros (the gradient buffers are torch.empty: a missed store leaks
    garbage), and so does every row of a Gaussian that no sub-pose saw"""
    for k, t in g.items():
        assert bool(torch.isfinite(t).all()), (what, k)
    beyond = g["sh"][:, nb:]
    assert torch.equal(beyond, torch.zeros_like(beyond)), (what, "sh gradient beyond the active bands")
    unseen = ~(radii > 0).any(dim=0)
    assert int(unseen.sum()) > 0, what
    for k in G_NAMES:
        rows = g[k][unseen]
        assert torch.equal(rows, torch.zeros_like(rows)), (what, k, "rows of Gaussians no sub-pose saw")


def _against_oracle(f, img, samples, g, what, dacc=None):
    """part-1 bars: per-sample images within IMG_ATOL off each sample's fragile pixels, the averaged image within 5e-4
    off the frame's, grad_el_ratio <= 1 for every tensor (sh without the colour-clamp-fragile rows)"""
    good = ~f["frag"]
    assert (samples.cpu().double() - f["samples"].detach())[~f["frag_s"]].abs().max().item() < IMG_ATOL, what
    assert (img.cpu().double() - f["ref"].detach())[good].abs().max().item() < 5e-4, what
    if dacc is not None:
        err = (dacc.cpu().double() - f["depth"].detach())[:, good].abs().max().item()
        assert err < 2e-4 * f["depth"].detach().max().item(), (what, err)        # test_gpu_depth_grad's bar
    keep = ~f["clamp_rows"]
    worst = {}
    for k in C.NAMES:
        g_hip, g_ref = g[k].cpu().numpy(), f["q"][k].grad.numpy()
        if k == "viewmat":
            g_hip, g_ref = g_hip[:3], g_ref[:3]
        if k == "sh":
            g_hip, g_ref = g_hip[keep.numpy()], g_ref[keep.numpy()]
        worst[k] = grad_el_ratio(g_hip, g_ref)
    print(f"[{what}] per-element gradient error / tolerance:", {k: round(v, 3) for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= 1.0, (what, k, v)
    return worst


def _oracle_case(oracle, deg, K, model="se3", depth=False):
    sc = C.scene(oracle, deg, K)
    f = C.oracle_frame(oracle, sc, deg, model, _oracle_depth if depth else None)
    t = C.tag(deg, K, model)
    check_fragile(f["frag"], t)          # (with the depth composite's pixels: they share the colour's thresholds)
    per_sample = float(f["frag_s"].float().mean())
    n_clamp = int(f["clamp_rows"].sum())
    print(f"[{t}] per sample image fragile {per_sample:.5f}; colours on the clamp {f['clamped']:.4f}; colour-clamp-fragile "
          f"rows {n_clamp} of {C.N}; smallest positive pre-clamp colour {f['min_pos']:.2e}")
    assert per_sample < 0.01, per_sample
    assert f["clamped"] >= C.CLAMPED_MIN, f["clamped"]
    assert n_clamp <= C.CLAMP_ROWS_MAX * C.N, n_clamp
    wt = C.loss_weights(f["frag"])
    wd = C.depth_weights(f["frag"]) if depth else None
    loss = (f["ref"] * wt.double()).sum()
    if depth:
        loss = loss + (f["depth"] * wd.double()).sum()
    loss.backward()
    nb = C.nb_of(deg)
    gsh = f["q"]["sh"].grad
    assert bool((gsh[:, nb:] == 0).all()) and bool((gsh[:, :nb].abs().amax(dim=(0, 2)) > 0).all())
    return sc, f, wt, wd


# --------------------------------------------------------------------------- 1. frame vs oracle, (degree, K) x layout
@pytest.mark.parametrize("deg,K", C.CASES)
def test_frame_vs_float64_oracle_at_every_degree_and_stride(gs, oracle, dev, deg, K):
    """S=3 x R=2 sub-poses, gamma 2.2, min-rgb 10, a background, the default gradient convention; DC x2 and rest x6 so
    that every band carries signal and the colour clamp is active (asserted: >= 2 % of the colours).  Both layouts —
    one [N,K,3] tensor with activated parameters; features_dc + features_rest with raw parameters (K = 1: the empty
    features_rest) — meet the baseline-config bars, unused bands and unseen rows are exact zeros, and the two layouts
    agree within test_raw_parameters_equal_activated_parameters' tolerance with the same non-zero rows.
    Launches (default route: sparse backward with zero fill): degree <= 3 -> project_fused_fwd_kernel<16,true>,
    slice_colors_kernel<16>, project_fused_bwd_sparse_kernel<16,true> with K_stride 1, 4, 9, 16 and 25 (nb < K_stride at
    (0,16), (1,16), (2,25), (3,25): the `b < nb` guards, and at K_stride 25 the tail loop past MAXB); (4,25) ->
    slice_colors_kernel<25> and project_fused_bwd_sparse_kernel<25,true>."""
    sc, f, wt, _ = _oracle_case(oracle, deg, K)
    nb = C.nb_of(deg)
    res = {}
    for layout in ("single", "split"):
        what = f"{C.tag(deg, K)} {layout}"
        img, samples, radii, _, g = _hip_frame(gs, dev, sc, deg, layout, wt=wt)
        _check_unused_bands_and_rows(g, radii, nb, what)
        _against_oracle(f, img, samples, g, what)
        res[layout] = (img, g)
    (img_a, g_a), (img_r, g_r) = res["single"], res["split"]
    images_close(img_r, img_a, 5e-6, f"{C.tag(deg, K)} split vs single layout", frac_max=2e-4)
    for k in G_NAMES:
        parts = {k: (g_a[k], g_r[k])}
        if k == "sh":
            parts = {"features_dc": (g_a[k][:, :1], g_r[k][:, :1])}
            if K > 1:
                parts["features_rest"] = (g_a[k][:, 1:nb], g_r[k][:, 1:nb])
        for name, (a, b) in parts.items():
            if a.numel() == 0:
                continue
            r = rel_max(b.cpu(), a.cpu())
            print(f"[kernel-vs-kernel {C.tag(deg, K)} layouts, grad {name}] rel_max = {r:.3e}")
            assert r < 2e-5, (name, r)
            rows_a = (a.reshape(C.N, -1) != 0).any(dim=1)
            rows_r = (b.reshape(C.N, -1) != 0).any(dim=1)
            assert torch.equal(rows_a, rows_r), (name, int((rows_a != rows_r).sum()))


# --------------------------------------------------------------------------- 2. the degree-4 instantiations, by route
@pytest.mark.parametrize("deg,K", [(4, 25), (3, 25), (1, 16)])
@pytest.mark.parametrize("knob,value", [("DEFER_COLOR", 0), ("GRAD_TUPLES", 0), ("SLICE_BASE", 4)])
def test_other_routes_give_the_default_result_at_other_degrees(gs, oracle, dev, deg, K, knob, value):
    """Routes of the degree dispatch the default frame does not take, each against the default route of the same scene
    (itself held to the oracle above): images bit for bit, gradients within the summation-order tolerance these routes
    have elsewhere (1e-4 of the tensor's maximum: DEFER_COLOR in test_every_runtime_knob_gives_the_default_result, the
    atomics backward in test_tuple_backward_equals_atomic_backward, another slicing in
    test_depth_sliced_equals_single_pass), unused bands and unseen rows exact zeros on both.
      DEFER_COLOR=0  SH in the projection: project_fused_fwd_kernel<25,false> at (4,25), <16,false> with nb < K_stride at
                     (3,25) / (1,16); its backward is project_fused_bwd_sparse_kernel<MAXB,true,false> through the Python
                     orchestration
      GRAD_TUPLES=0  fp32 atomics into v_records, no `touched` flags: the DENSE project_fused_bwd_kernel<25,false> at
                     (4,25); at (3,25) project_fused_bwd_kernel<16,false> with K_stride 25, whose tail loop zeroes the bands the
                     instantiation does not hold
      SLICE_BASE=4   several depth slices (asserted: >= 2 non-empty): gs_slice_colors (slice_colors_kernel<25> at
                     (4,25)) runs once per slice
    The non-zero-fill forms project_fused_bwd_sparse_kernel<.,false,.> and the dense depth form
    project_fused_bwd_kernel<.,true> have no caller in the Python package (ops passes the zero-fill flag whenever it has
    `touched` flags, and the frame backend without them has no depth channel): only a C caller reaches them."""
    from gsdeblur_amd import ops
    sc = C.scene(oracle, deg, K)
    wt = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(5))
    nb = C.nb_of(deg)
    res = {}
    old = getattr(ops, knob)
    try:
        for v in (old, value):
            setattr(ops, knob, v)
            img, samples, radii, _, g = _hip_frame(gs, dev, sc, deg, "single", wt=wt)
            _check_unused_bands_and_rows(g, radii, nb, f"{C.tag(deg, K)} {knob}={v}")
            if knob == "SLICE_BASE" and v == value:
                assert sum(1 for x in ops.last_slice_intersects if x > 0) >= 2
            res[v] = (samples, g)
    finally:
        setattr(ops, knob, old)
    a, b = res[old], res[value]
    assert torch.equal(a[0], b[0])
    for k in a[1]:
        assert rel_max(b[1][k].cpu(), a[1][k].cpu()) < 1e-4, (knob, k)


def test_degree_4_depth_gradient_vs_oracle(gs, oracle, dev):
    """return_depth=True with a depth term in the loss: project_fused_bwd_sparse_kernel<25,true,true>, against the
    oracle's depth composite (test_gpu_depth_grad._oracle_depth), at the bars of part 1"""
    sc, f, wt, wd = _oracle_case(oracle, 4, 25, depth=True)
    for layout in ("single", "split"):
        img, samples, radii, dacc, g = _hip_frame(gs, dev, sc, 4, layout, wt=wt, wd=wd)
        _check_unused_bands_and_rows(g, radii, 25, f"depth {layout}")
        _against_oracle(f, img, samples, g, f"{C.tag(4, 25)} depth {layout}", dacc)


def test_degree_4_pixel_velocity_model_vs_oracle(gs, oracle, dev):
    """motion_model pixel_velocity at degree 4 (gs_project_pixvel_fwd / _bwd: the <25> instantiations with the
    pixel-velocity branch, colour from the mid-exposure pose) against the oracle's pixel-velocity mode, part-1 bars"""
    sc, f, wt, _ = _oracle_case(oracle, 4, 25, model="pixel_velocity")
    for layout in ("single", "split"):
        img, samples, radii, _, g = _hip_frame(gs, dev, sc, 4, layout, model="pixel_velocity", wt=wt)
        _check_unused_bands_and_rows(g, radii, 25, f"pixvel {layout}")
        _against_oracle(f, img, samples, g, f"{C.tag(4, 25, 'pixvel')} {layout}")


def _combined(gs, dev, sc, deg, vms, leaves, **kw):
    return gs.render_combined(leaves["means"], leaves["log_scales"], leaves["quats"], leaves["opacity_logits"],
                              leaves["dc"], vms, C.BG.to(dev), S, R, sc["fx"], sc["fy"], sc["cx"], sc["cy"], H, W,
                              gamma=C.GAMMA, min_rgb_level=C.MLEVEL, sh_degree=deg, sh_rest=leaves["rest"],
                              raw_params=True, **kw)


def _leaves(sc, dev, grad=True):
    p = {k: sc[k].float().to(dev).clone().requires_grad_(grad) for k in C.NAMES if k != "sh"}
    sh = sc["sh"].float().to(dev)
    p["dc"] = sh[:, 0, :].clone().requires_grad_(grad)
    p["rest"] = sh[:, 1:, :].clone().requires_grad_(grad)
    return p


def test_degree_4_render_batch_equals_two_render_combined(gs, oracle, dev):
    """B = 2 cameras at degree 4 in one frame: image, alphas, radii bit for bit the two single-camera frames; the batch's
    Gaussian gradients are the sum of the two single backwards up to fp32 summation order (2e-5, the bar
    test_every_runtime_knob_gives_the_default_result has for it)"""
    sc = C.scene(oracle, 4, 25)
    times, _, _ = gs.subpose_schedule(S, C.ET, R, C.RT)
    tt = torch.tensor(times, device=dev)
    wt = torch.rand(2, H, W, 3, generator=torch.Generator().manual_seed(5)).to(dev)
    V = sc["viewmat"].float().to(dev)
    lin, ang = sc["lin_vel"].float().to(dev), sc["ang_vel"].float().to(dev)
    vms = torch.stack([gs.subpose_viewmats(V, lin, ang, tt), gs.subpose_viewmats(V, -1.5 * lin, 0.5 * ang, tt + 0.01)])
    p = _leaves(sc, dev)
    rgb, al, radii = gs.render_batch(p["means"], p["log_scales"], p["quats"], p["opacity_logits"], p["dc"], vms,
                                     C.BG.to(dev), S, R, sc["fx"], sc["fy"], sc["cx"], sc["cy"], H, W, gamma=C.GAMMA,
                                     min_rgb_level=C.MLEVEL, sh_degree=4, sh_rest=p["rest"], raw_params=True)
    (rgb * wt).sum().backward()
    q = _leaves(sc, dev)
    for b in range(2):
        r1, a1, ra1 = _combined(gs, dev, sc, 4, vms[b], q)
        assert torch.equal(rgb[b].detach(), r1.detach()) and torch.equal(al[b], a1) and torch.equal(radii[b], ra1), b
        (r1 * wt[b]).sum().backward()
    for k in ("means", "log_scales", "quats", "opacity_logits", "dc", "rest"):
        assert bool(torch.isfinite(p[k].grad).all()) and float(p[k].grad.abs().max()) > 0, k
        assert rel_max(p[k].grad.cpu(), q[k].grad.cpu()) < 2e-5, k


@pytest.mark.parametrize("deg,K", [(1, 16), (4, 25)])
def test_render_step_equals_autograd_route_at_other_degrees(gs, oracle, dev, deg, K):
    """step.render_step (what train_step uses) against render_combined + backward with features_dc / features_rest and
    raw parameters, as test_render_step_equals_autograd_route: image and Gaussian gradients bit for bit, camera
    gradients to 1e-5; at (1,16) the 12 unused bands of features_rest are exact zeros on both routes"""
    sc = C.scene(oracle, deg, K)
    times, _, _ = gs.subpose_schedule(S, C.ET, R, C.RT)
    tt = torch.tensor(times, device=dev)
    wt = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(4)).to(dev)
    p = _leaves(sc, dev)
    vms = gs.subpose_viewmats(p["viewmat"], p["lin_vel"], p["ang_vel"], tt)
    rgb, _, _ = _combined(gs, dev, sc, deg, vms, p, return_alpha=False)
    rgb.backward(wt)
    q = _leaves(sc, dev, grad=False)
    rgb2, g, radii = gs.render_step(q["means"], q["log_scales"], q["quats"], q["opacity_logits"], q["dc"], q["viewmat"],
                                    q["lin_vel"], q["ang_vel"], tt, C.BG.to(dev), S, R, sc["fx"], sc["fy"], sc["cx"],
                                    sc["cy"], H, W, lambda img: wt, gamma=C.GAMMA, min_rgb_level=C.MLEVEL, sh_degree=deg,
                                    sh_rest=q["rest"], raw_params=True)
    assert torch.equal(rgb2, rgb.detach()) and radii.shape == (S * R, C.N)
    for k, name in (("means", "means"), ("log_scales", "scales"), ("quats", "quats"), ("opacity_logits", "opacities"),
                    ("dc", "sh"), ("rest", "sh_rest")):
        assert torch.equal(g[name], p[k].grad), k
    for k in ("viewmat", "lin_vel", "ang_vel"):
        assert rel_max(g[k].cpu(), p[k].grad.cpu()) < 1e-5, k
    beyond = g["sh_rest"][:, C.nb_of(deg) - 1:]
    assert torch.equal(beyond, torch.zeros_like(beyond)) and float(g["sh_rest"].abs().max()) > 0


# --------------------------------------------------------------------------- 3. model and training at other degrees
def _camera(gs, sc, idx=0, lin=(0.3, 0.1, 0.0), ang=(0.0, 0.2, 0.1)):
    c2w = torch.eye(4)[:3].clone()
    c2w[:, 1] *= -1
    c2w[:, 2] *= -1                        # OpenGL camera looking down the oracle scene's +z
    return gs.Camera(c2w, sc["fx"], sc["fy"], sc["cx"], sc["cy"], W, H,
                     metadata=dict(cam_idx=idx, camera_linear_velocity=list(lin), camera_angular_velocity=list(ang),
                                   exposure_time=1 / 60, rolling_shutter_time=0.0))


def _target(gs, oracle, dev, sc, cfg, cam):
    """the scene's own render, from a copy of the scene with other DC colours removed: a target the start can approach"""
    with torch.no_grad():
        return gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev).get_outputs_for_camera(cam)["rgb"].detach()


def _perturbed(sc, seed=1):
    g = torch.Generator().manual_seed(seed)
    start = dict(sc)
    K = sc["sh"].shape[1]
    start["sh"] = sc["sh"] + 0.3 * torch.randn(sc["sh"].shape, generator=g) * (torch.arange(K) == 0)[None, :, None]
    return start


@pytest.mark.parametrize("degree,interval,steps", [(3, 2, 8), (4, 1, 6)])
def test_progressive_sh_schedule(gs, oracle, dev, degree, interval, steps):
    """sh_degree_interval: the active degree is min(step // interval, sh_degree) while training, so the kernels run with
    nb < K_stride on the model's own route (render_step, features_dc + features_rest, raw parameters).  After each step
    features_rest.grad beyond the active bands is exactly zero and those bands' parameters are bit-unchanged until
    their degree activates; in eval mode the full degree renders."""
    K = (degree + 1) ** 2
    sc = C.scene(oracle, degree, K)
    cfg = gs.SplatfactoDeblurConfig(sh_degree=degree, sh_degree_interval=interval, blur_samples=3, gamma=2.2,
                                    min_rgb_level=0.0, rolling_shutter_compensation=False)
    cam = _camera(gs, sc)
    full = gs.SplatfactoDeblurConfig(sh_degree=degree, blur_samples=3, gamma=2.2, min_rgb_level=0.0,
                                     rolling_shutter_compensation=False)
    gt = _target(gs, oracle, dev, sc, full, cam)
    model = gs.SplatfactoDeblurModel.from_scene(cfg, _perturbed(sc), dev)
    opts = gs.training.make_optimizers(model, lr_scale=10.0)
    assert gs.training.one_call_route(model)
    rest0 = model.features_rest.detach().clone()
    seen = []
    for it in range(steps):
        model.train()
        deg = model.active_sh_degree()
        seen.append(deg)
        st = gs.training.train_step(model, opts, cam, gt, 0.2)
        assert math.isfinite(st["loss"])
        nb = (deg + 1) ** 2
        gr = model.features_rest.grad
        assert gr.shape == (C.N, K - 1, 3) and bool(torch.isfinite(gr).all())
        assert torch.equal(gr[:, nb - 1:], torch.zeros_like(gr[:, nb - 1:])), (it, deg)
        if deg > 0:
            assert float(gr[:, (deg ** 2) - 1:nb - 1].abs().max()) > 0, (it, deg)        # the newest band is trained
        assert torch.equal(model.features_rest.detach()[:, nb - 1:], rest0[:, nb - 1:]), (it, deg)
        if deg > 0:
            assert not torch.equal(model.features_rest.detach()[:, :nb - 1], rest0[:, :nb - 1])
    assert seen == [min(i // interval, degree) for i in range(steps)], seen
    # eval renders every band whatever the step: the same image as a model without the schedule
    model2 = gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev)
    model2.step = 0
    model2.eval()
    assert model2.active_sh_degree() == degree
    with torch.no_grad():
        assert torch.equal(model2.get_outputs(cam)["rgb"], gt)
        model2.train()
        assert model2.active_sh_degree() == 0
        assert not torch.equal(model2.get_outputs(cam)["rgb"], gt)


@pytest.mark.parametrize("degree", [0, 4])
@pytest.mark.parametrize("optimizer,mask", [("adam", "visible"), ("selective_adam", "visible"),
                                            ("selective_adam", "touched")])
def test_model_trains_at_degree_0_and_4(gs, oracle, dev, degree, optimizer, mask):
    """features_rest is [N,0,3] (a null data pointer) at degree 0 and [N,24,3] (72 floats per row) at degree 4: both go
    through get_outputs, five train_steps with the dense and the selective optimizer under both masks (every selective
    step against a dense HipAdam step of the selected rows, bit for bit, as tests/test_gpu_selective_adam.py) and a batch
    render.  Before this change gs_adam_step_rows refused widths 0 and > 64 and gs_dp_row_mask (the "touched" mask) a
    zero-width tensor: the first selective step raised HipLibraryError."""
    from test_gpu_selective_adam import _check_selective_step, _expected_mask, _snapshot
    K = (degree + 1) ** 2
    sc = C.scene(oracle, degree, K)
    cfg = gs.SplatfactoDeblurConfig(sh_degree=degree, blur_samples=3, gamma=2.2, min_rgb_level=0.0,
                                    rolling_shutter_compensation=False, optimizer=optimizer, selective_mask=mask)
    cam = _camera(gs, sc)
    gt = _target(gs, oracle, dev, sc, cfg, cam)
    model = gs.SplatfactoDeblurModel.from_scene(cfg, _perturbed(sc), dev, num_cameras=2)
    assert model.features_rest.shape == (C.N, K - 1, 3)
    model.eval()
    with torch.no_grad():
        out = model.get_outputs(cam)
    assert out["rgb"].shape == (H, W, 3) and bool(torch.isfinite(out["rgb"]).all())
    opts = gs.training.make_optimizers(model, lr_scale=10.0)
    losses = []
    for it in range(5):
        snap = _snapshot(model, opts)
        st = gs.training.train_step(model, opts, cam, gt, 0.2)
        losses.append(st["loss"])
        assert model.features_rest.grad.shape == (C.N, K - 1, 3)
        if optimizer == "selective_adam" and it > 0:
            _check_selective_step(gs, model, opts, snap, _expected_mask(model, mask))
    print(f"degree {degree} {optimizer}/{mask}: losses", [round(v, 5) for v in losses])
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0], losses
    for k, prm in model.gauss_params().items():
        assert bool(torch.isfinite(prm).all()), k
        stt = opts[k].state[prm]
        assert stt["exp_avg"].shape == prm.shape and bool(torch.isfinite(stt["exp_avg_sq"]).all()), k
    model.eval()
    with torch.no_grad():
        ob = model.get_outputs_batch([cam, _camera(gs, sc, 1, lin=(-0.2, 0.0, 0.1))])
    assert ob["rgb"].shape == (2, H, W, 3) and bool(torch.isfinite(ob["rgb"]).all())


@pytest.mark.timeout(1800)            # as test_training_with_absgrad_densification_end_to_end (450 iterations; here 250)
@pytest.mark.parametrize("degree", [0, 4])
def test_training_with_densification_at_degree_0_and_4(gs, dev, tmp_path, degree):
    """a short train_scene on the self-generated dataset with selective Adam and the refinement schedule: split,
    duplicate and cull carry the zero-width / 72-wide features_rest rows and their Adam moments"""
    import synthetic_dataset as SD
    from gsdeblur_amd import densify as D
    root = str(tmp_path / "ds")
    SD.generate(root, dev, width=160, height=112, n_frames=12, n_gaussians=4000, speed=1.0, dense_samples=16,
                seed_points=1000)
    scene = gs.load_transforms(root)
    images = gs.data.load_scene_images(scene, dev)
    xyz, rgb = gs.load_seed_points_ply(scene.ply_file_path)
    iters = 250
    dcfg = D.DensifyConfig(warmup_length=100, refine_every=100, reset_alpha_every=8, stop_split_at=iters,
                           stop_screen_size_at=200)
    cfg = gs.SplatfactoDeblurConfig(sh_degree=degree, blur_samples=5, gamma=2.2, min_rgb_level=0.0,
                                    rolling_shutter_compensation=False, use_scale_regularization=True,
                                    optimizer="selective_adam")
    model = SD.init_from_seed_points(cfg, xyz, rgb, dev, num_cameras=len(scene.cameras))
    n0, K = model.num_points, (degree + 1) ** 2
    r = gs.training.train_scene(model, scene, images, iters, densify=dcfg, log_every=1)
    losses = [float(h["loss"]) for h in r["history"]]
    assert len(losses) == iters and iters // dcfg.refine_every - 1 >= 1            # a refinement at step 200
    print("degree", degree, "gaussians", n0, "->", model.num_points, "loss", sum(losses[:20]) / 20, "->",
          sum(losses[-20:]) / 20, "psnr", r["results"]["psnr"])
    assert all(math.isfinite(v) for v in losses)
    assert model.num_points != n0
    assert model.features_rest.shape == (model.num_points, K - 1, 3)
    assert sum(losses[-20:]) / 20 < sum(losses[:20]) / 20
    for prm in model.gauss_params().values():
        assert bool(torch.isfinite(prm).all())


ROW_WIDTHS = [0, 1, 3, 45, 64, 65, 72, 192]


@pytest.mark.parametrize("density", [0.0, 0.004, 0.5, 1.0])
def test_adam_step_rows_at_every_row_width(gs, dev, density):
    """gs_adam_step_rows through fused.adam_step_all(row_mask=...) on rows of 0 (an empty [N,0,3] tensor), 1, 3, 45, 64,
    65, 72 ([N,24,3]) and 192 floats, all in ONE launch: the selected rows equal a dense gs_adam_step of the same
    tensors bit for bit — parameter and both moments, the guarantee the kernel states —, masked-off rows are
    bit-unchanged, over three steps with changing masks."""
    from gsdeblur_amd.fused import HipAdam, adam_step_all
    N = 4099
    g = torch.Generator(device=dev).manual_seed(11)
    shapes = [(N, 0, 3), (N, 1), (N, 3), (N, 15, 3), (N, 64), (N, 65), (N, 24, 3), (N, 192)]
    assert [math.prod(s[1:]) for s in shapes] == ROW_WIDTHS
    ps = [torch.nn.Parameter(torch.randn(s, device=dev, generator=g)) for s in shapes]
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opts = [HipAdam([p], lr=1e-3 * (i + 1), eps=1e-15, selective=True) for i, p in enumerate(ps)]
    ref = [HipAdam([q], lr=1e-3 * (i + 1), eps=1e-15) for i, q in enumerate(qs)]
    for step in range(3):
        mask = torch.rand(N, device=dev, generator=g) < density if 0.0 < density < 1.0 else \
            torch.full((N,), density == 1.0, dtype=torch.bool, device=dev)
        for p, q in zip(ps, qs):
            p.grad = torch.randn(p.shape, device=dev, generator=g) * 0.1
            q.grad = p.grad.clone()
        before = [(p.detach().clone(), {k: v.clone() for k, v in o.state[p].items() if torch.is_tensor(v)})
                  for p, o in zip(ps, opts)]
        adam_step_all(opts, row_mask=mask)
        adam_step_all(ref)
        torch.cuda.synchronize()
        for i, (p, q) in enumerate(zip(ps, qs)):
            st, rst = opts[i].state[p], ref[i].state[q]
            assert st["step"] == step + 1 and p.shape == shapes[i]
            for got, want, was in ((p.detach(), q.detach(), before[i][0]),
                                   (st["exp_avg"], rst["exp_avg"], before[i][1].get("exp_avg")),
                                   (st["exp_avg_sq"], rst["exp_avg_sq"], before[i][1].get("exp_avg_sq"))):
                assert torch.equal(got[mask], want[mask]), (i, step, "selected rows differ from gs_adam_step")
                was = torch.zeros_like(got) if was is None else was
                assert torch.equal(got[~mask], was[~mask]), (i, step, "masked-off rows changed")
            with torch.no_grad():                     # keep the dense reference in lock step with the selective state
                q.copy_(p)
                rst["exp_avg"].copy_(st["exp_avg"])
                rst["exp_avg_sq"].copy_(st["exp_avg_sq"])


def test_adam_step_rows_c_abi_skips_zero_width_and_null_pointers(gs, dev):
    """the C entry itself: a zero-width tensor is skipped even with null pointers (what an empty torch tensor hands over),
    a launch of nothing but zero-width tensors is a no-op, a negative width is refused"""
    L = gs._lib.load()
    N = 1000
    vp = ctypes.c_void_p
    t = [torch.randn(N, 72, device=dev) for _ in range(4)]
    t[3] = t[3].abs()
    orig = [x.clone() for x in t]
    mask = (torch.arange(N, device=dev) % 3 == 0)
    ws_bytes = L.gs_adam_step_rows_workspace_bytes(N)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    stream = vp(torch.cuda.current_stream().cuda_stream)

    def call(widths, ptrs):
        n = len(widths)
        arr = [(vp * n)(*[p[j] for p in ptrs]) for j in range(4)]
        return L.gs_adam_step_rows(n, N, vp(mask.view(torch.uint8).data_ptr()), arr[0], arr[1], arr[2], arr[3],
                                   (ctypes.c_int * n)(*widths), (ctypes.c_float * n)(*([1e-3] * n)), 0.9, 0.999, 1e-15, 1,
                                   vp(ws.data_ptr()), ws_bytes, stream)
    null = [None] * 4
    real = [x.data_ptr() for x in t]
    assert call([0], [null]) == 0 and call([0, 0], [null, null]) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(t, orig))
    assert call([-1], [real]) == 1 and call([72, -1], [real, null]) == 1
    assert call([72], [null]) == 1                                 # a tensor with columns needs its pointers
    assert call([0, 72], [null, real]) == 0
    torch.cuda.synchronize()
    assert torch.equal(t[1], orig[1])                              # the gradient is never written
    for j in (0, 2, 3):
        assert torch.equal(t[j][~mask], orig[j][~mask]) and not torch.equal(t[j][mask], orig[j][mask])


def test_dp_row_kernels_with_zero_width_and_72_wide_tensors(gs, dev):
    """gs_dp_row_mask / gs_dp_pack_rows / gs_dp_scatter_add_rows / gs_dp_pack_masked_rows / gs_dp_scatter_add_payload on
    the gradient shapes of a degree-0 model (features_rest [N,0,3]: no payload column, a null pointer) and of a degree-4
    model ([N,24,3]): bit for bit what the torch ops give, as test_dp_row_kernels_match_torch and
    test_dp_masked_pack_and_payload_scatter_match_torch"""
    from gsdeblur_amd.dp import _RowOps
    N = 20011
    for rest in ((N, 0, 3), (N, 24, 3)):
        shapes = [(N, 3), (N, 3), (N, 4), (N,), (N, 3), rest]
        world = 3
        gens = [torch.Generator().manual_seed(900 + r) for r in range(world)]
        rank_grads = []
        for r in range(world):
            touched = torch.rand(N, generator=gens[r]) < 0.03
            rank_grads.append([torch.randn(s, generator=gens[r]) * touched.view(-1, *([1] * (len(s) - 1))) for s in shapes])
        payloads, counts = [], []
        for r in range(world):
            cpu = _RowOps([x.clone() for x in rank_grads[r]])
            hip = _RowOps([x.clone().to(dev) for x in rank_grads[r]])
            assert hip.wtot == cpu.wtot == 14 + math.prod(rest[1:])
            m_cpu, m_hip = cpu.row_mask(), hip.row_mask()
            assert torch.equal(m_cpu, m_hip.cpu()) and 0 < int(m_cpu.sum()) < N
            idx = m_cpu.nonzero().reshape(-1)
            Mpad = idx.numel() + 7
            p_cpu, p_hip = cpu.pack(idx, Mpad), hip.pack(idx.to(dev), Mpad)
            assert torch.equal(p_cpu.view(torch.int32), p_hip.cpu().view(torch.int32))
            payloads.append(p_cpu)
            counts.append(idx.numel())
            # the fixed-capacity form: header, rows and indices, capacity above and below the row count
            total = idx.numel()
            for cap in (total + 100, total // 2):
                pay_c, pay_h = cpu.pack_masked(cap), hip.pack_masked(cap)
                M = min(total, cap)
                assert torch.equal(pay_c[:1 + M].view(torch.int32), pay_h[:1 + M].cpu().view(torch.int32)), cap
                assert pay_h[0, :2].view(torch.int32).tolist() == [total, min(total, cap)]
                acc_c = _RowOps([torch.zeros(s) for s in shapes])
                acc_h = _RowOps([torch.zeros(s, device=dev) for s in shapes])
                acc_c.scatter_add_payload(pay_c, cap, 0.5)
                acc_h.scatter_add_payload(pay_h, cap, 0.5)
                for a, b, s in zip(acc_c.grads, acc_h.grads, shapes):
                    assert b.shape == s and torch.equal(a, b.cpu())
        acc_cpu = _RowOps([torch.zeros(s) for s in shapes])
        acc_hip = _RowOps([torch.zeros(s, device=dev) for s in shapes])
        for r in range(world):
            acc_cpu.scatter_add(payloads[r], counts[r], 1.0 / world)
            acc_hip.scatter_add(payloads[r].to(dev), counts[r], 1.0 / world)
        for a, b, i in zip(acc_cpu.grads, acc_hip.grads, range(len(shapes))):
            assert torch.equal(a, b.cpu()), i
            want = sum(rank_grads[r][i] for r in range(world)) / world
            assert torch.allclose(a, want, atol=1e-6)
