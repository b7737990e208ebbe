"""Bilateral-grid colour correction on the MI355X: gs_bilagrid_slice_fwd / gs_bilagrid_slice_bwd / gs_bilagrid_tv_fwd_bwd
against the float64 grid_sample reference (tests/bilagrid_reference.py), run-to-run determinism, the autograd Function
against its two halves, train_step's two routes, and the feature-off path.

Tolerance — measured, not chosen: per output, 4 x the largest error that torch's own float32 evaluation of the REFERENCE
makes against float64 on the same inputs (the kernels sum in another order than torch, hence the factor), plus a floor of
1e-6 x max |reference|.  Both errors are printed.  The guide gradient jumps where luma * (L - 1) crosses an integer:
pixels within 1e-4 of one leave the v_rgb comparison only, at most 0.1 % of an input's pixels (asserted)."""
import numpy as np
import pytest
import torch

import bilagrid_reference as R

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (7, 5), (64, 48), (480, 270), (1920, 1080)]      # (W, H)
SHAPES = [(16, 16, 8), (4, 6, 2), (2, 2, 2)]                      # (GW, GH, L)


def rel_max(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def check_against_reference(got, grids, rgb, idx, v_out, what):
    L = grids.shape[2]
    ref = R.slice_ref_grads(grids, rgb, idx, v_out)
    ref32 = R.slice_ref_grads(grids, rgb, idx, v_out, dtype=torch.float32)
    frag = R.fragile_pixels(rgb, L)
    n_frag, n_px = int(frag.sum()), frag.numel()
    assert n_frag <= 1e-3 * n_px, f"{what}: {n_frag} of {n_px} pixels are fragile"
    keep = (~frag)[..., None].expand_as(rgb)
    for name, g, r, r32, mask in (("out", got[0], ref[0], ref32[0], None), ("v_rgb", got[1], ref[1], ref32[1], keep),
                                  ("v_grids", got[2], ref[2], ref32[2], None)):
        e_torch = (r32.double() - r).abs()
        e_ours = (g.cpu().double() - r).abs()
        if mask is not None:
            e_torch, e_ours = e_torch[mask], e_ours[mask]
        bound = 4.0 * float(e_torch.max()) + 1e-6 * float(r.abs().max())
        print(f"{what} {name}: kernel {float(e_ours.max()):.3e}, torch fp32 {float(e_torch.max()):.3e}, "
              f"bound {bound:.3e}, max|ref| {float(r.abs().max()):.3e}, fragile {n_frag}/{n_px}")
        assert float(e_ours.max()) <= bound, (what, name, float(e_ours.max()), bound)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("size", SIZES)
def test_kernels_against_the_grid_sample_reference(gs, dev, size, shape):
    W, H = size
    seed = 300 + 10 * SIZES.index(size) + SHAPES.index(shape)
    for B, G, idx in ((1, 1, [0]), (3, 3, [2, 0, 2])):                 # grid 1 of the second case is selected by nobody
        grids, rgb, v_out = R.random_case(B, H, W, G, shape, seed + B)
        gd, rd, vd = grids.to(dev), rgb.to(dev), v_out.to(dev)
        out = gs.bilagrid.slice_fwd(gd, rd, idx)
        v_rgb, v_grids = gs.bilagrid.slice_bwd(gd, rd, idx, vd)
        torch.cuda.synchronize()
        if G == 3:
            assert float(v_grids[1].abs().max()) == 0.0                # every row is stored, zeros included
        check_against_reference((out, v_rgb, v_grids), grids, rgb, idx, v_out, f"{W}x{H} {shape} B={B}")


@pytest.mark.parametrize("shape", SHAPES)
def test_tv_kernel_against_the_sliced_reference(gs, dev, shape):
    for G in (1, 5):
        grids, _, _ = R.random_case(1, 1, 1, G, shape, 40 + G)
        weight = 10.0
        gd = grids.to(dev)
        v = torch.zeros_like(gd)
        value = gs.bilagrid.tv_fwd_bwd_hip(gd, weight, v)
        again = gs.bilagrid.tv_fwd_bwd_hip(gd, weight, v)                 # the gradient is accumulated
        ref_v, ref_g = R.tv_ref_grads(grids, weight)
        ref32_v, ref32_g = R.tv_ref_grads(grids, weight, dtype=torch.float32)
        b_v = 4 * abs(float(ref32_v) - float(ref_v)) + 1e-6 * abs(float(ref_v))
        b_g = 4 * float((ref32_g.double() - ref_g).abs().max()) + 1e-6 * float(ref_g.abs().max())
        e_v = abs(float(value) - float(ref_v))
        e_g = float((0.5 * v.cpu().double() - ref_g).abs().max())
        print(f"tv {shape} G={G}: value err {e_v:.3e} (torch fp32 {abs(float(ref32_v) - float(ref_v)):.3e}, bound "
              f"{b_v:.3e}), grad err {e_g:.3e} (bound {b_g:.3e})")
        assert torch.equal(value, again)
        assert e_v <= b_v and e_g <= b_g
        # the autograd form: same value, same gradient
        p = gd.clone().requires_grad_(True)
        t = gs.bilagrid.tv_loss(p, weight)
        t.backward()
        assert torch.equal(t.detach(), value) and torch.equal(p.grad, 0.5 * v)


@pytest.mark.parametrize("size", [(64, 48), (1920, 1080)])
def test_two_backward_runs_are_bit_identical_and_the_function_equals_its_halves(gs, dev, size):
    W, H = size
    grids, rgb, v_out = R.random_case(3, H, W, 2, (16, 16, 8), 9)
    gd, rd, vd = grids.to(dev), rgb.to(dev), v_out.to(dev)
    idx = [1, 0, 1]
    a = gs.bilagrid.slice_bwd(gd, rd, idx, vd)
    b = gs.bilagrid.slice_bwd(gd, rd, idx, vd)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    gp, rp = gd.clone().requires_grad_(True), rd.clone().requires_grad_(True)
    out = gs.bilagrid.slice(gp, rp, idx)
    out.backward(vd)
    assert torch.equal(out.detach(), gs.bilagrid.slice_fwd(gd, rd, idx))
    assert torch.equal(rp.grad, a[0]) and torch.equal(gp.grad, a[1])
    one = gs.bilagrid.slice(gd, rd[1], 0)                                 # the single-image form
    assert one.shape == rd[1].shape and torch.equal(one, out.detach()[1])
    dev_idx = torch.tensor(idx, dtype=torch.int32, device=dev)            # a device index tensor
    assert torch.equal(gs.bilagrid.slice_fwd(gd, rd, dev_idx), out.detach())


def _scene_and_camera(gs, n, W, H, seed):
    sc = gs.data.synthetic_scene(n, W, H, sh_degree=3, seed=seed)
    sc["lin_vel"], sc["ang_vel"] = sc["lin_vel"] * 20, sc["ang_vel"] * 10
    c2w = torch.eye(4)[:3].clone()
    c2w[:, 1] *= -1
    c2w[:, 2] *= -1
    flip = torch.tensor([1.0, -1.0, -1.0])
    cam = gs.Camera(c2w, sc["fx"], sc["fy"], sc["cx"], sc["cy"], W, H,
                    metadata=dict(cam_idx=1, camera_linear_velocity=[float(v) for v in sc["lin_vel"] * flip],
                                  camera_angular_velocity=[float(v) for v in sc["ang_vel"] * flip],
                                  exposure_time=1 / 60, rolling_shutter_time=0.0))
    return sc, cam


def test_train_step_routes_agree_with_the_grid(gs, dev):
    """the one-call route (slice forward -> loss -> slice backward inside grad_image, TV through the kernel's own
    accumulation) and the autograd route (get_outputs + loss.backward()): same loss, PSNR, Gaussian and grid gradients,
    same parameters after two steps — at the tolerance of tests/test_gpu_parity.py::test_train_step_routes_agree"""
    from gsdeblur_amd import train_step as T
    n, W, H, S = 6000, 128, 96, 3
    sc, cam = _scene_and_camera(gs, n, W, H, 31)
    target = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(5)).to(dev)
    results = []
    saved = T.TRAIN_AUTOGRAD
    try:
        for autograd_route in (0, 1):
            T.TRAIN_AUTOGRAD = autograd_route
            cfg = gs.SplatfactoDeblurConfig(blur_samples=S, rolling_shutter_compensation=False, gamma=2.2, min_rgb_level=10.0,
                                            use_bilateral_grid=True)
            model = gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev, num_cameras=3)
            with torch.no_grad():                                        # away from the identity: every term is alive
                model.bilateral_grids.add_(0.05 * torch.randn(model.bilateral_grids.shape,
                                                              generator=torch.Generator().manual_seed(2)).to(dev))
            assert T.one_call_route(model) == (not autograd_route)
            opts = T.make_optimizers(model)
            assert type(opts["bilateral_grid"]).__name__ == "HipAdam"
            h = [T.train_step(model, opts, cam, target, 0.2) for _ in range(2)]
            grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
            params = {k: p.detach().clone() for k, p in model.named_parameters()}
            results.append((h, grads, params))
    finally:
        T.TRAIN_AUTOGRAD = saved
    (h0, g0, p0), (h1, g1, p1) = results
    assert set(g0) == set(g1) and {"means", "scales", "quats", "opacities", "features_dc", "features_rest",
                                   "bilateral_grids"} <= set(g0)
    for a, b in zip(h0, h1):
        assert abs(a["loss"] - b["loss"]) < 1e-6 * max(1.0, abs(b["loss"])) and abs(a["psnr"] - b["psnr"]) < 1e-4
    for k in g0:
        assert float(g0[k].abs().max()) > 0, k
        print(f"routes {k}: grad {rel_max(g0[k].cpu(), g1[k].cpu()):.2e}, param {rel_max(p0[k].cpu(), p1[k].cpu()):.2e}")
        assert rel_max(g0[k].cpu(), g1[k].cpu()) < 2e-5, k
        assert rel_max(p0[k].cpu(), p1[k].cpu()) < 2e-5, k
    moved = (p0["bilateral_grids"] != gs.bilagrid.identity_grids(3).to(dev)).flatten(1).any(1)
    assert moved.tolist() == [True, True, True]


def test_batch_route_and_eval_renders_with_the_grid(gs, dev):
    n, W, H = 4000, 96, 64
    sc, cam = _scene_and_camera(gs, n, W, H, 12)
    cfg = gs.SplatfactoDeblurConfig(blur_samples=2, rolling_shutter_compensation=False, use_bilateral_grid=True)
    model = gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev, num_cameras=2)
    with torch.no_grad():
        model.bilateral_grids[1, [0, 5, 10]] = 0.5
    plain = model.get_outputs_for_camera(cam)["rgb"]
    model.train()
    assert torch.allclose(model.get_outputs(cam)["rgb"].detach(), 0.5 * plain, atol=1e-6)
    assert torch.allclose(model.get_outputs(cam, bilateral_grid=False)["rgb"].detach(), plain, atol=1e-6)
    cam0 = gs.Camera(cam.camera_to_world, cam.fx, cam.fy, cam.cx, cam.cy, W, H, metadata=dict(cam.metadata, cam_idx=0))
    out = model.get_outputs_batch([cam, cam0])["rgb"].detach()
    assert torch.allclose(out[0], 0.5 * plain, atol=1e-6) and torch.allclose(out[1], plain, atol=1e-6)
    assert torch.equal(model.get_outputs_for_cameras([cam, cam0])["rgb"][0], plain)
    opts = gs.training.make_optimizers(model)
    target = (plain * 0.8).contiguous()
    h = gs.training.train_step(model, opts, [cam, cam0], [target, target], 0.2)
    assert np.isfinite(h["loss"]) and model.bilateral_grids.grad is not None
    assert float(model.bilateral_grids.grad[0].abs().max()) > 0 and float(model.bilateral_grids.grad[1].abs().max()) > 0
    bad = gs.Camera(cam.camera_to_world, cam.fx, cam.fy, cam.cx, cam.cy, W, H, metadata=dict(cam.metadata, cam_idx=2))
    with pytest.raises(ValueError, match="cam_idx"):
        gs.training.train_step(model, opts, bad, target, 0.2)


def test_feature_off_calls_none_of_the_new_entry_points(gs, dev, monkeypatch):
    n, W, H = 3000, 96, 64
    sc, cam = _scene_and_camera(gs, n, W, H, 4)
    lib = gs._lib.load()
    calls = []
    names = ("gs_bilagrid_slice_fwd", "gs_bilagrid_slice_bwd", "gs_bilagrid_slice_bwd_workspace_bytes",
             "gs_bilagrid_tv_fwd_bwd", "gs_bilagrid_tv_workspace_bytes")

    class Spy:
        """stands in for the ctypes.CDLL handle: forwards everything, records the new entry points"""
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name in names:
                return lambda *a: (calls.append(name), fn(*a))[1]
            return fn
    monkeypatch.setattr(gs._lib, "_lib", Spy())
    target = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(5)).to(dev)
    cfg = gs.SplatfactoDeblurConfig(blur_samples=2, rolling_shutter_compensation=False)
    model = gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev, num_cameras=2)
    assert model.bilateral_grids is None
    opts = gs.training.make_optimizers(model)
    gs.training.train_step(model, opts, cam, target, 0.2)
    gs.training.train_step(model, opts, [cam, cam], [target, target], 0.2)
    model.get_outputs_for_camera(cam)
    assert calls == []
    cfg_on = gs.SplatfactoDeblurConfig(blur_samples=2, rolling_shutter_compensation=False, use_bilateral_grid=True)
    model_on = gs.SplatfactoDeblurModel.from_scene(cfg_on, sc, dev, num_cameras=2)
    gs.training.train_step(model_on, gs.training.make_optimizers(model_on), cam, target, 0.2)
    assert {"gs_bilagrid_slice_fwd", "gs_bilagrid_slice_bwd", "gs_bilagrid_tv_fwd_bwd"} <= set(calls)   # the spy sees them
