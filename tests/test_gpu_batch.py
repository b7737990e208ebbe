"""Batched cameras on the GPU: ops.render_batch renders B cameras x S blur samples x R row bands as ONE frame of
B*S*R sub-poses (gs_frame_desc.cameras = B).  Forward against the per-camera render_combined (bit for bit), backward
against the float64 oracle per camera and against the single-camera backward, B = 1 against render_combined, a
sequence of batches through one FrameHints, the full-size scene, and the model / evaluation / training surfaces."""
import math
import types

import pytest
import torch

from test_gpu_parity import grad_el_ratio
from test_gpu_depth_grad import _oracle_depth

pytestmark = pytest.mark.gpu

G_NAMES = ["means", "log_scales", "quats", "opacity_logits", "sh"]


def _scene(gs, n, W, H, seed, profile="survey"):
    sc = gs.data.synthetic_scene(n, W, H, sh_degree=3, seed=seed, profile=profile)
    sc["lin_vel"], sc["ang_vel"] = sc["lin_vel"] * 20, sc["ang_vel"] * 10
    return sc


def _pose(gs, V, shift, rot):
    """V moved by a twist (the sub-pose map at t = 1), computed on the GPU, returned on the CPU"""
    d = torch.device("cuda:0")
    return gs.subpose_viewmats(V.float().to(d), shift.to(d), rot.to(d), torch.ones(1, device=d))[0].detach().cpu()


def _cameras(gs, sc, B, seed=0):
    """B distinct cameras about the scene's own: pose, velocity scale / sign and exposure differ per camera.
    -> [(viewmat [4,4], lin [3], ang [3], exposure_time)] on the CPU"""
    cams = []
    for b in range(B):
        ph = 2.0 * math.pi * (b + 0.37 * seed) / max(B, 1)
        shift = torch.tensor([0.10 * math.cos(ph), 0.06 * math.sin(ph), 0.05 * (b % 3)])
        rot = torch.tensor([0.06 * math.cos(ph), 0.10 * math.sin(ph), 0.02 * ((b % 4) - 1.5)])
        V = _pose(gs, sc["viewmat"], shift, rot)
        k = (1.0 + 0.2 * (b % 5)) * (-1.0 if b % 2 else 1.0)
        cams.append((V, sc["lin_vel"].float() * k, sc["ang_vel"].float() * k, (1.0 + 0.25 * b) / 60))
    return cams


def _viewmats(gs, cam, S, R, dev, rs_time=1 / 30, params=None):
    V, lin, ang, et = cam
    if params is not None:
        V, lin, ang = params
    times, _, _ = gs.subpose_schedule(S, et, R, rs_time)
    return gs.subpose_viewmats(V.to(dev), lin.to(dev), ang.to(dev), torch.tensor(times, device=dev))


def _gauss(sc, dev, grad=False):
    return {k: sc[k].float().to(dev).requires_grad_(grad) for k in G_NAMES}


def _args(p):
    return (p["means"], p["log_scales"].exp(), p["quats"], torch.sigmoid(p["opacity_logits"]), p["sh"])


def _forward_equal(gs, dev, sc, cams, S, R, H, W, hints=None):
    p = _gauss(sc, dev)
    vms = torch.stack([_viewmats(gs, c, S, R, dev) for c in cams])
    with torch.no_grad():
        rgb, al, radii, dacc = gs.render_batch(*_args(p), vms, None, S, R, sc["fx"], sc["fy"], sc["cx"], sc["cy"], H, W,
                                               gamma=2.2, min_rgb_level=10.0, return_depth=True, hints=hints)
        for b in range(len(cams)):
            r1, a1, ra1, d1 = gs.render_combined(*_args(p), vms[b], None, S, R, sc["fx"], sc["fy"], sc["cx"], sc["cy"],
                                                 H, W, gamma=2.2, min_rgb_level=10.0, return_depth=True)
            assert torch.equal(rgb[b], r1), b
            assert torch.equal(al[b], a1), b
            assert torch.equal(dacc[b], d1), b
            assert torch.equal(radii[b], ra1), b
    return rgb


@pytest.mark.parametrize("R", [1, 10])
def test_batch_forward_equals_per_camera_renders(gs, dev, R):
    W, H, S = 256, 192, 5
    sc = _scene(gs, 20000, W, H, 11)
    _forward_equal(gs, dev, sc, _cameras(gs, sc, 4), S, R, H, W)


def test_batch_forward_with_several_depth_slices(gs, dev):
    from gsdeblur_amd import ops
    W, H, S = 256, 192, 5
    sc = _scene(gs, 60000, W, H, 12, profile="trained")
    old = ops.SLICE_BASE
    try:
        ops.SLICE_BASE = 2
        _forward_equal(gs, dev, sc, _cameras(gs, sc, 4), S, 1, H, W)
        vms = torch.stack([_viewmats(gs, c, S, 1, dev) for c in _cameras(gs, sc, 4)])
        with torch.no_grad():
            gs.render_batch(*_args(_gauss(sc, dev)), vms, None, S, 1, sc["fx"], sc["fy"], sc["cx"], sc["cy"], H, W)
        assert sum(1 for x in ops.last_slice_intersects if x > 0) >= 2
    finally:
        ops.SLICE_BASE = old


def _backward_vs_oracle(gs, O, dev, loss_kind, learn_bg, W, H, n, S, R, B):
    sc = O.synthetic_scene(n, W, H, seed=41, scale_mult=6.0)
    sc["lin_vel"], sc["ang_vel"] = sc["lin_vel"] * 20, sc["ang_vel"] * 10
    cams = _cameras(gs, sc, B, seed=1)
    gamma, mlevel = 2.2, 10.0
    p = {k: sc[k].float().to(dev).requires_grad_(True) for k in G_NAMES}
    cp = [tuple(t.to(dev).requires_grad_(True) for t in c[:3]) for c in cams]
    vms = torch.stack([_viewmats(gs, cams[b], S, R, dev, params=cp[b]) for b in range(B)])
    bg0 = torch.tensor([0.2, 0.5, 0.7])
    bg = bg0.to(dev).requires_grad_(True) if learn_bg else None
    rgb, _, _, dacc = gs.render_batch(*_args(p), vms, bg, S, R, sc["fx"], sc["fy"], sc["cx"], sc["cy"], H, W,
                                      gamma=gamma, min_rgb_level=mlevel, return_depth=True)
    q = {k: sc[k].double().requires_grad_(True) for k in G_NAMES}
    cq = [tuple(t.double().requires_grad_(True) for t in c[:3]) for c in cams]
    qbg = bg0.double().requires_grad_(True) if learn_bg else None
    loss_ref = 0.0
    loss_lib = 0.0
    for b in range(B):
        cfg = O.RenderConfig(H, W, sc["fx"], sc["fy"], sc["cx"], sc["cy"], blur_samples=S, rs_bands=R,
                             exposure_time=cams[b][3], rolling_shutter_time=1 / 30, gamma=gamma, min_rgb_level=mlevel)
        out, _, _, frag, parts, _ = O.render(cfg, q["means"], q["log_scales"].exp(), q["quats"],
                                             torch.sigmoid(q["opacity_logits"]), q["sh"], cq[b][0], cq[b][1], cq[b][2],
                                             background=qbg, return_parts=True)
        if loss_kind == "rgb+depth":
            dref, dfrag = _oracle_depth(O, cfg, parts)
            frag = frag | dfrag
        err = (rgb[b].detach().cpu().double() - out.detach())[~frag].abs().max().item()
        assert err < 5e-4, (b, err)
        wc = torch.rand(out.shape, generator=torch.Generator().manual_seed(7 + b), dtype=torch.float64) - 0.5
        wc[frag] = 0.0
        wc = wc * (2.0 / (H * W))
        loss_ref = loss_ref + (wc * out).sum()
        loss_lib = loss_lib + (wc.float().to(dev) * rgb[b]).sum()
        if loss_kind == "rgb+depth":
            wd = torch.rand(dref.shape, generator=torch.Generator().manual_seed(17 + b), dtype=torch.float64) - 0.5
            wd[:, frag] = 0.0
            wd = wd / (H * W)
            loss_ref = loss_ref + (wd * dref).sum()
            loss_lib = loss_lib + (wd.float().to(dev) * dacc[b]).sum()
    loss_ref.backward()
    loss_lib.backward()
    torch.cuda.synchronize()
    ratios = {}
    for k in G_NAMES:
        ratios[k] = grad_el_ratio(p[k].grad.cpu().numpy(), q[k].grad.numpy())
    for b in range(B):
        for j, name in enumerate(("viewmat", "lin_vel", "ang_vel")):
            ref, got = cq[b][j].grad, cp[b][j].grad.cpu()
            if name == "viewmat":
                ref, got = ref[:3], got[:3]
            ratios[f"{name}[{b}]"] = grad_el_ratio(got.numpy(), ref.numpy())
    if learn_bg:
        ratios["background"] = grad_el_ratio(bg.grad.cpu().numpy(), qbg.grad.numpy())
    print("grad_el_ratio", ratios)
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("loss_kind,learn_bg", [("rgb", False), ("rgb+depth", False), ("rgb", True)])
def test_batch_backward_matches_oracle(gs, oracle, dev, loss_kind, learn_bg):
    _backward_vs_oracle(gs, oracle, dev, loss_kind, learn_bg, W=128, H=96, n=3000, S=3, R=2, B=3)


@pytest.mark.parametrize("loss_kind", ["rgb", "rgb+depth"])
def test_batch_backward_in_several_slices_matches_oracle(gs, oracle, dev, loss_kind):
    """a slice budget that forces several depth slices: the backward compositor of a frame of several cameras carries its
    reverse-traversal state from slice to slice (raster_bwd_sload_kernel<true, 1, DEPTH, false, true>).  4 x 3 tiles, two
    cameras of two samples each, so that the camera of sample image s is s / 2"""
    from gsdeblur_amd import ops
    old = ops.SLICE_BASE
    try:
        ops.SLICE_BASE = 2
        _backward_vs_oracle(gs, oracle, dev, loss_kind, False, W=64, H=48, n=400, S=2, R=1, B=2)
        assert sum(1 for x in ops.last_slice_intersects if x > 0) >= 2
    finally:
        ops.SLICE_BASE = old


def _batch_grads(gs, dev, sc, cams, S, R, H, W, wc):
    p = _gauss(sc, dev, grad=True)
    cp = [tuple(t.to(dev).requires_grad_(True) for t in c[:3]) for c in cams]
    vms = torch.stack([_viewmats(gs, cams[b], S, R, dev, params=cp[b]) for b in range(len(cams))])
    xy = torch.zeros(len(cams), sc["means"].shape[0], 2, device=dev)
    rgb, _, _ = gs.render_batch(*_args(p), vms, None, S, R, sc["fx"], sc["fy"], sc["cx"], sc["cy"], H, W, gamma=2.2,
                                min_rgb_level=10.0, xy_grad_out=xy)
    (wc * rgb).sum().backward()
    torch.cuda.synchronize()
    return {k: p[k].grad.clone() for k in G_NAMES}, [[t.grad.clone() for t in c] for c in cp], xy.clone()


def _single_grads(gs, dev, sc, cam, S, R, H, W, wc):
    p = _gauss(sc, dev, grad=True)
    cp = tuple(t.to(dev).requires_grad_(True) for t in cam[:3])
    xy = torch.zeros(sc["means"].shape[0], 2, device=dev)
    rgb, _, _ = gs.render_combined(*_args(p), _viewmats(gs, cam, S, R, dev, params=cp), None, S, R, sc["fx"], sc["fy"],
                                   sc["cx"], sc["cy"], H, W, gamma=2.2, min_rgb_level=10.0, xy_grad_out=xy)
    (wc * rgb).sum().backward()
    torch.cuda.synchronize()
    return {k: p[k].grad.clone() for k in G_NAMES}, [t.grad.clone() for t in cp], xy.clone()


def test_batch_backward_matches_single_camera_backwards(gs, dev):
    W, H, S, R, B = 256, 192, 5, 1, 4
    sc = _scene(gs, 20000, W, H, 13)
    cams = _cameras(gs, sc, B, seed=2)
    wc = (torch.rand(B, H, W, 3, generator=torch.Generator().manual_seed(5)) - 0.5).to(dev) / (H * W)
    gb, cb, xyb = _batch_grads(gs, dev, sc, cams, S, R, H, W, wc)
    total = None
    for b in range(B):
        g1, c1, xy1 = _single_grads(gs, dev, sc, cams[b], S, R, H, W, wc[b])
        total = g1 if total is None else {k: total[k] + g1[k] for k in G_NAMES}
        for j in range(3):
            assert grad_el_ratio(cb[b][j].cpu().numpy(), c1[j].cpu().numpy()) <= 1.0, (b, j)
        assert grad_el_ratio(xyb[b].cpu().numpy(), xy1.cpu().numpy()) <= 1.0, b
        assert torch.count_nonzero(xy1) > 0
    for k in G_NAMES:
        assert grad_el_ratio(gb[k].cpu().numpy(), total[k].cpu().numpy()) <= 1.0, k
    # determinism: a second run of the batch gives every gradient bit for bit
    gb2, cb2, xyb2 = _batch_grads(gs, dev, sc, cams, S, R, H, W, wc)
    assert all(torch.equal(gb[k], gb2[k]) for k in G_NAMES)
    assert all(torch.equal(a, c) for x, y in zip(cb, cb2) for a, c in zip(x, y))
    assert torch.equal(xyb, xyb2)


def test_batch_of_one_is_render_combined_bit_for_bit(gs, dev):
    W, H, S, R = 256, 192, 5, 2
    sc = _scene(gs, 20000, W, H, 14)
    cam = _cameras(gs, sc, 1, seed=3)[0]
    wc = (torch.rand(1, H, W, 3, generator=torch.Generator().manual_seed(6)) - 0.5).to(dev) / (H * W)
    gb, cb, xyb = _batch_grads(gs, dev, sc, [cam], S, R, H, W, wc)
    g1, c1, xy1 = _single_grads(gs, dev, sc, cam, S, R, H, W, wc[0])
    assert all(torch.equal(gb[k], g1[k]) for k in G_NAMES)
    assert all(torch.equal(a, c) for a, c in zip(cb[0], c1))
    assert torch.equal(xyb[0], xy1)
    _forward_equal(gs, dev, sc, [cam], S, R, H, W)


def test_batch_sequence_through_one_hints_with_adaptive_default(gs, dev):
    from gsdeblur_amd import ops
    W, H, S = 256, 192, 5
    sc = _scene(gs, 60000, W, H, 15, profile="trained")
    cams = _cameras(gs, sc, 16, seed=4)
    saved = (ops.SLICE_ADAPT, ops.SLICE_BASE)
    try:
        ops.SLICE_ADAPT, ops.SLICE_BASE = 1, 64
        hints = ops.FrameHints()
        for cycle in range(3):
            for k in range(0, 16, 4):
                if cycle < 2:
                    vms = torch.stack([_viewmats(gs, c, S, 1, dev) for c in cams[k:k + 4]])
                    with torch.no_grad():
                        gs.render_batch(*_args(_gauss(sc, dev)), vms, None, S, 1, sc["fx"], sc["fy"], sc["cx"],
                                        sc["cy"], H, W, gamma=2.2, min_rgb_level=10.0, hints=hints)
                else:
                    _forward_equal(gs, dev, sc, cams[k:k + 4], S, 1, H, W, hints=hints)
        assert hints.frames >= 12
    finally:
        ops.SLICE_ADAPT, ops.SLICE_BASE = saved


def test_batch_full_size(gs, dev):
    W, H, S, B = 1920, 1080, 5, 4
    sc = gs.data.synthetic_scene(1_000_000, W, H, sh_degree=3, seed=1234)
    cams = _cameras(gs, sc, B, seed=5)
    _forward_equal(gs, dev, sc, cams, S, 1, H, W)
    p = _gauss(sc, dev, grad=True)
    cp = [tuple(t.to(dev).requires_grad_(True) for t in c[:3]) for c in cams]
    vms = torch.stack([_viewmats(gs, cams[b], S, 1, dev, params=cp[b]) for b in range(B)])
    rgb, _, _ = gs.render_batch(*_args(p), vms, None, S, 1, sc["fx"], sc["fy"], sc["cx"], sc["cy"], H, W, gamma=2.2,
                                min_rgb_level=10.0)
    rgb.mean().backward()
    torch.cuda.synchronize()
    for k in G_NAMES:
        assert torch.isfinite(p[k].grad).all() and torch.count_nonzero(p[k].grad) > 0, k
    for c in cp:
        assert all(torch.isfinite(t.grad).all() for t in c)


def _views(gs, sc, W, H, n, exposure=1 / 60):
    """n cameras (gs.Camera, OpenGL c2w) about the scene's view, with data velocities and exposures of their own"""
    V = sc["viewmat"].float()
    cams = []
    for i in range(n):
        ph = 2.0 * math.pi * i / n
        Vi = _pose(gs, V, torch.tensor([0.08 * math.cos(ph), 0.05 * math.sin(ph), 0.0]),
                   torch.tensor([0.04 * math.cos(ph), 0.06 * math.sin(ph), 0.0]))
        c2w_cv = torch.linalg.inv(Vi.double()).float()
        c2w = c2w_cv[:3].clone()
        c2w[:, 1:3] *= -1.0                                    # OpenCV -> OpenGL camera axes
        k = 1.0 + 0.2 * (i % 3)
        cams.append(gs.Camera(c2w, sc["fx"], sc["fy"], sc["cx"], sc["cy"], W, H,
                              metadata={"cam_idx": i, "exposure_time": exposure * k,
                                        "camera_linear_velocity": (sc["lin_vel"] * k * (-1) ** i).tolist(),
                                        "camera_angular_velocity": (sc["ang_vel"] * k).tolist()}))
    return cams


def test_model_batch_equals_get_outputs_and_evaluate(gs, dev):
    W, H = 192, 128
    sc = _scene(gs, 20000, W, H, 16)
    cfg = gs.SplatfactoDeblurConfig(sh_degree=3, blur_samples=5, gamma=2.2, min_rgb_level=10.0,
                                    rolling_shutter_compensation=False)
    model = gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev, num_cameras=8)
    cams = _views(gs, sc, W, H, 8)
    out = model.get_outputs_for_cameras(cams[:4])
    for b in range(4):
        one = model.get_outputs_for_camera(cams[b])
        assert torch.equal(out["rgb"][b], one["rgb"]), b
        assert torch.equal(out["accumulation"][b], one["accumulation"]), b
        assert torch.equal(out["depth"][b], one["depth"]), b
    images = [model.get_outputs_for_camera(c)["rgb"].clamp(0, 1) * 0.9 + 0.05 for c in cams]
    a = gs.training.evaluate(model, cams, images, list(range(8)))
    b = gs.training.evaluate(model, cams, images, list(range(8)), batch_size=4)
    assert a == b


def test_train_scene_in_batches_lowers_the_loss(gs, dev):
    W, H = 128, 96
    sc = _scene(gs, 3000, W, H, 17)
    cams = _views(gs, sc, W, H, 8)
    cfg = gs.SplatfactoDeblurConfig(sh_degree=3, blur_samples=3, gamma=2.2, min_rgb_level=0.0,
                                    rolling_shutter_compensation=False)
    gt = gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev, num_cameras=8)
    with torch.no_grad():
        images = [gt.get_outputs_for_camera(c)["rgb"].clamp(0, 1).contiguous() for c in cams]
    g = torch.Generator().manual_seed(1)
    start = dict(sc)
    start["sh"] = sc["sh"] + 0.2 * torch.randn(sc["sh"].shape, generator=g) * (torch.arange(16) == 0)[None, :, None]
    start["means"] = sc["means"] + 0.01 * torch.randn(sc["means"].shape, generator=g)
    model = gs.SplatfactoDeblurModel.from_scene(cfg, start, dev, num_cameras=8)
    scene = types.SimpleNamespace(cameras=cams, train_indices=list(range(8)), eval_indices=[0, 4])
    before = gs.training.evaluate(model, cams, images, scene.eval_indices, batch_size=4)["psnr"]
    r = gs.training.train_scene(model, scene, images, 60, batch_size=4, log_every=1, seed=2)
    hist = [h["loss"] for h in r["history"]]
    print("batched training: psnr", before, "->", r["results"]["psnr"], "loss", hist[0], "->", hist[-1])
    assert sum(hist[-5:]) / 5 < 0.8 * sum(hist[:5]) / 5
    assert r["results"]["psnr"] > before + 1.0
