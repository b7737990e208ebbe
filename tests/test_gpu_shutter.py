"""Learnable exposure / readout times on the GPU: gs_subpose_viewmats_bwd_times against float64 autograd through
matrix_exp (and its 22 camera floats against gs_subpose_viewmats_bwd_store, bit for bit), the chain from an image cotangent
to d loss / d times on both routes, "off is off", the batch route, and recovery of known exposure and readout times from
rolling-shutter frames."""
import math

import pytest
import torch

import shutter_reference as SR

pytestmark = pytest.mark.gpu


def _camera_of_the_parity_test(oracle):
    # V0, lin, ang of tests/test_gpu_parity.py::test_subpose_viewmats_fwd_bwd
    V0 = oracle.subpose_viewmats(torch.eye(4, dtype=torch.float64), torch.tensor([0.3, -0.2, 0.5], dtype=torch.float64),
                                 torch.tensor([0.2, 0.4, -0.1], dtype=torch.float64), [1.0])[0].float()
    return V0, torch.tensor([0.1, 0.05, -0.2]), torch.tensor([0.05, -0.08, 0.03])


# ---- 1. kernel vs reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zero_ang", [False, True])
@pytest.mark.parametrize("P", [1, 5, 50, 256])
def test_times_gradient_vs_float64_and_old_tangents_bit_unchanged(gs, oracle, dev, P, zero_ang):
    """P = 256 (MAX_SUBPOSES): 19 * 256 items, 19 loop trips per thread of the one block"""
    V0, lin, ang = _camera_of_the_parity_test(oracle)
    if zero_ang:
        ang = torch.zeros(3)
    g = torch.Generator().manual_seed(P)
    times = torch.tensor([0.0]) if P == 1 else torch.cat([torch.tensor([-0.02, -0.01, 0.0, 0.01, 0.3]),
                                                          (torch.rand(P - 5, generator=g) - 0.5) * 0.2])
    go = torch.randn(P, 4, 4, generator=g)
    go[:, 3, :] = 0
    res = []
    for with_times in (True, False):
        Vd, ld, ad = (t.to(dev).requires_grad_(True) for t in (V0, lin, ang))
        td = times.to(dev).requires_grad_(with_times)
        out = gs.subpose_viewmats(Vd, ld, ad, td)
        (out * go.to(dev)).sum().backward()
        res.append((Vd.grad, ld.grad, ad.grad, td.grad))
    (vV, vl, va, vt), (vV0, vl0, va0, none) = res
    assert none is None and tuple(vt.shape) == (P,)
    # the 18 camera tangents: the bits of the call that does not ask for the time gradient
    assert torch.equal(vV, vV0) and torch.equal(vl, vl0) and torch.equal(va, va0)
    gt = SR.gradients(V0, lin, ang, times.double(), go)[3]
    r = SR.rel_max(vt, gt)
    print(f"P {P} zero_ang {zero_ang}: times.grad rel_max {r:.3g}")
    assert float(gt.abs().max()) > 1e-3 and r < 1e-5


def test_times_entry_validates_its_arguments(gs, dev):
    L = gs._lib.load()
    buf = torch.zeros(64, device=dev)
    p = buf.data_ptr()
    INVALID = L.gs_subpose_viewmats_bwd_times(0, p, p, p, p, p, p, p, p, p, None)
    assert INVALID != 0
    for k in range(4):
        outs = [p, p, p, p]
        outs[k] = None
        assert L.gs_subpose_viewmats_bwd_times(1, p, p, p, p, p, *outs, None) == INVALID


# ---- 2. chain --------------------------------------------------------------------------------------------------------
def _small_scene(gs, dev, n=300, W=48, H=32, seed=5):
    sc = gs.data.synthetic_scene(n, W, H, sh_degree=1, seed=seed, scale_mult=6.0)
    sc["lin_vel"], sc["ang_vel"] = sc["lin_vel"] * 20, sc["ang_vel"] * 10
    q = {k: sc[k].float().to(dev) for k in ("means", "log_scales", "quats", "opacity_logits", "sh", "viewmat", "lin_vel",
                                              "ang_vel")}
    return sc, q


def test_chain_from_the_image_to_the_times_on_both_routes(gs, dev):
    W, H, S, R = 48, 32, 3, 2
    sc, q = _small_scene(gs, dev, 300, W, H)
    times = torch.tensor(gs.subpose_schedule(S, 1 / 30, R, 1 / 40)[0], device=dev).requires_grad_(True)
    v_img = torch.randn(H, W, 3, generator=torch.Generator().manual_seed(9)).to(dev)
    dc, rest = q["sh"][:, 0, :].contiguous(), q["sh"][:, 1:, :].contiguous()
    geom = (sc["fx"], sc["fy"], sc["cx"], sc["cy"], H, W)
    vms = gs.subpose_viewmats(q["viewmat"], q["lin_vel"], q["ang_vel"], times)
    vms.retain_grad()
    rgb = gs.render_combined(q["means"], q["log_scales"], q["quats"], q["opacity_logits"], dc, vms, None, S, R, *geom,
                             gamma=2.2, min_rgb_level=10.0, sh_degree=1, sh_rest=rest, raw_params=True)[0]
    (rgb * v_img).sum().backward()
    assert float(vms.grad.abs().max()) > 0
    want = SR.gradients(q["viewmat"].cpu(), q["lin_vel"].cpu(), q["ang_vel"].cpu(), times.detach().cpu().double(),
                        vms.grad.cpu())[3]
    r = SR.rel_max(times.grad, want)
    print(f"chain: times.grad rel_max {r:.3g}, |grad| max {float(want.abs().max()):.3g}")
    assert float(want.abs().max()) > 0 and r < 1e-5
    args = (q["means"], q["log_scales"], q["quats"], q["opacity_logits"], dc, q["viewmat"], q["lin_vel"], q["ang_vel"],
            times.detach(), None, S, R, *geom, v_img)
    kw = dict(gamma=2.2, min_rgb_level=10.0, sh_degree=1, sh_rest=rest)
    _, g, _ = gs.render_step(*args, times_grad=True, **kw)
    assert torch.equal(g["times"], times.grad)
    _, g_off, _ = gs.render_step(*args, **kw)
    assert set(g_off) == {"means", "scales", "quats", "opacities", "sh", "sh_rest", "viewmat", "lin_vel", "ang_vel",
                          "background"}
    assert set(g) == set(g_off) | {"times"}
    for k in g_off:
        assert (g[k] is None and g_off[k] is None) or torch.equal(g[k], g_off[k]), k
    _, g_only, _ = gs.render_step(*args, times_grad=True, camera_grads=False, **kw)
    assert torch.equal(g_only["times"], times.grad) and g_only["viewmat"] is None
    with pytest.raises(ValueError, match="times_grad"):
        gs.render_step(*args, times_grad=True, motion_model="pixel_velocity", **kw)


# ---- 3. off is off ---------------------------------------------------------------------------------------------------
def test_off_is_off_on_both_routes(gs, dev, monkeypatch):
    """a model with the optimizer off against the rendering the project had before it — the cached host schedule
    model._const(times) handed to subpose_viewmats / render_step, spelled out here: torch.equal parameters and gradients
    after two training steps on the one-call route and on the autograd route, and no times gradient asked of render_step"""
    from gsdeblur_amd import step as STEP, train_step as T
    n, W, H, S, R = 2000, 96, 64, 3, 2
    sc = gs.data.synthetic_scene(n, W, H, sh_degree=2, seed=31)
    sc["lin_vel"], sc["ang_vel"] = sc["lin_vel"] * 20, sc["ang_vel"] * 10
    c2w = torch.eye(4)[:3].clone()
    c2w[:, 1] *= -1
    c2w[:, 2] *= -1
    flip = torch.tensor([1.0, -1.0, -1.0])
    cam = gs.Camera(c2w, sc["fx"], sc["fy"], sc["cx"], sc["cy"], W, H,
                    metadata=dict(cam_idx=0, camera_linear_velocity=[float(v) for v in sc["lin_vel"] * flip],
                                  camera_angular_velocity=[float(v) for v in sc["ang_vel"] * flip],
                                  exposure_time=1 / 60, rolling_shutter_time=1 / 50))
    target = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(5)).to(dev)
    seen = []
    real_step = STEP.render_step

    def spy(*a, **kw):
        seen.append(("times_grad" in kw, a[8]))
        rgb, g, radii = real_step(*a, **kw)
        assert "times" not in g
        return rgb, g, radii
    monkeypatch.setattr(STEP, "render_step", spy)

    def run(autograd_route, as_before):
        cfg = gs.SplatfactoDeblurConfig(sh_degree=2, blur_samples=S, rolling_shutter_compensation=True, rs_bands=R,
                                        gamma=2.2, min_rgb_level=10.0, background_color="auto")
        cfg.camera_optimizer.mode = "SO3xR3"
        cfg.camera_velocity_optimizer.enabled = True
        model = gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev)
        assert model.exposure_adjustment is None and model.readout_adjustment is None
        if as_before:
            # the schedule and its upload as they were: metadata -> host floats -> _const
            monkeypatch.setattr(model, "_base_times", lambda c: (float(c.metadata.get("exposure_time", 0.0)),
                                                                 float(c.metadata.get("rolling_shutter_time", 0.0))),
                                raising=False)
            monkeypatch.setattr(model, "_times_tensor", lambda c, S_, R_, times: model._const(times), raising=False)
        monkeypatch.setattr(T, "TRAIN_AUTOGRAD", autograd_route)
        assert T.one_call_route(model) == (not autograd_route)
        opts = T.make_optimizers(model)
        assert "camera_shutter_opt" not in opts
        for _ in range(2):
            T.train_step(model, opts, cam, target, 0.2)
        return ({k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None},
                {k: p.detach().clone() for k, p in model.named_parameters()}, model)

    for autograd_route in (0, 1):
        seen.clear()
        g_new, p_new, model = run(autograd_route, False)
        g_old, p_old, _ = run(autograd_route, True)
        assert set(g_new) == set(g_old) and set(p_new) == set(p_old) and "pose_adjustment" in g_new
        for k in g_new:
            assert torch.equal(g_new[k], g_old[k]), (autograd_route, k)
        for k in p_new:
            assert torch.equal(p_new[k], p_old[k]), (autograd_route, k)
        assert len(seen) == (0 if autograd_route else 4) and not any(flag for flag, _ in seen)
        if not autograd_route:
            host = model._schedule(cam)[2]
            assert all(t is model._const(host) or torch.equal(t, model._const(host)) for _, t in seen)


# ---- 4. batch --------------------------------------------------------------------------------------------------------
def test_batch_route_sums_the_cameras_gradients(gs, dev):
    n, W, H, S, R = 1500, 96, 64, 3, 2
    sc = gs.data.synthetic_scene(n, W, H, sh_degree=1, seed=13)
    sc["lin_vel"], sc["ang_vel"] = sc["lin_vel"] * 20, sc["ang_vel"] * 10
    flip = torch.tensor([1.0, -1.0, -1.0])
    cams = []
    for b in range(2):
        c2w = torch.eye(4)[:3].clone()
        c2w[:, 1] *= -1
        c2w[:, 2] *= -1
        c2w[0, 3] = 0.05 * b
        k = (1.0, -1.3)[b]
        cams.append(gs.Camera(c2w, sc["fx"], sc["fy"], sc["cx"], sc["cy"], W, H,
                              metadata=dict(cam_idx=b, camera_linear_velocity=[float(v) * k for v in sc["lin_vel"] * flip],
                                            camera_angular_velocity=[float(v) * k for v in sc["ang_vel"] * flip],
                                            exposure_time=(1 + b) / 60, rolling_shutter_time=1 / (40 + 10 * b))))
    cfg = gs.SplatfactoDeblurConfig(sh_degree=1, blur_samples=S, rolling_shutter_compensation=True, rs_bands=R, gamma=2.2,
                                    min_rgb_level=10.0)
    cfg.camera_shutter_optimizer.exposure = cfg.camera_shutter_optimizer.readout = "global"
    model = gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev, num_cameras=2).train()
    with torch.no_grad():
        model.exposure_adjustment.fill_(0.2)
        model.readout_adjustment.fill_(-0.3)
    w = torch.randn(2, H, W, 3, generator=torch.Generator().manual_seed(4)).to(dev)
    out = model.get_outputs_batch(cams)
    (out["rgb"] * w).sum().backward()
    ge, gr = model.exposure_adjustment.grad.clone(), model.readout_adjustment.grad.clone()
    se, sr = torch.zeros_like(ge), torch.zeros_like(gr)
    for b in range(2):
        model.exposure_adjustment.grad = model.readout_adjustment.grad = None
        (model.get_outputs(cams[b])["rgb"] * w[b]).sum().backward()
        se += model.exposure_adjustment.grad
        sr += model.readout_adjustment.grad
    print("batch:", ge.tolist(), se.tolist(), gr.tolist(), sr.tolist())
    assert float(se.abs().max()) > 0 and float(sr.abs().max()) > 0
    assert SR.rel_max(ge, se) < 1e-5 and SR.rel_max(gr, sr) < 1e-5


# ---- 5. recovery -----------------------------------------------------------------------------------------------------
RECOVERY_FRAMES = 4
# passes through the frames per start: 600 steps.  Adam moves a log-time by at most ~lr per step, so the group's rate
# (training.SHUTTER_LR = 1e-3) needs >= 347 steps to bring a 2x error inside ln(2)/2; 600 leaves room for the slowdown
# near the optimum (the rate was chosen on this budget).  About 0.6 s per start on an MI355X.
RECOVERY_ITERATIONS = 150


@pytest.fixture(scope="module")
def truth(gs, dev):
    import shutter_recovery_check as RC          # tools/ (conftest puts it on sys.path)
    return RC.ground_truth(dev, RECOVERY_FRAMES)


@pytest.mark.parametrize("which", ["exposure", "readout", "joint"])
def test_shutter_optimizer_recovers_known_times_from_rolling_shutter_frames(gs, dev, truth, which):
    """ground-truth Gaussians as constants, the true data velocities, targets from the independent per-pixel-row ground
    truth at exposure = readout = 1/15, cameras whose metadata is off by 0.5x / 2x, one global adjustment per learned
    time.  Every learned time must end closer to the truth than to its start in log space, |ln(learned / true)| <
    ln(2) / 2 — the S = 5 midpoint rule widens a box exposure by 1 / sqrt(1 - 1/S^2), about 2 %, far inside that; the
    loss falls on every frame and the Gaussians receive no gradient."""
    import shutter_recovery_check as RC
    bound = 0.5 * math.log(2.0)
    for e_mult, r_mult in RC.STARTS[which]:
        r = RC.recover(dev, truth, which, e_mult, r_mult, RECOVERY_ITERATIONS)
        print(f"{which} start E x{e_mult:g} T x{r_mult:g}: learned/true exposure {r['exposure_ratio']:.3f} readout "
              f"{r['readout_ratio']:.3f}; loss " + " ".join(f"{r['first'][i]:.4f}->{r['last'][i]:.4f}" for i in r["first"]))
        if e_mult != 1.0:
            assert abs(math.log(r["exposure_ratio"])) < bound, r
        else:
            assert r["exposure_ratio"] == pytest.approx(1.0, rel=1e-6)       # not learned: the metadata value
        if r_mult != 1.0:
            assert abs(math.log(r["readout_ratio"])) < bound, r
        else:
            assert r["readout_ratio"] == pytest.approx(1.0, rel=1e-6)
        for i in r["first"]:
            assert r["last"][i] < r["first"][i], (i, r["first"][i], r["last"][i])
        assert r["gauss_grads"] == []
