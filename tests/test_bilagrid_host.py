"""Bilateral-grid colour correction on the CPU: csrc/bilagrid_math.h compiled with g++ against the float64 grid_sample
reference (tests/bilagrid_reference.py), the torch restatement of bilagrid.py against the same reference, the model /
training surface with a stand-in render, a grid-only fit, a world-2 gloo run, and the C-ABI entries.

Tolerance of the float32 comparisons (the rule of tests/test_gpu_bilagrid.py): per output, 4 x the largest error that
torch's own float32 evaluation of the REFERENCE makes against float64 on the same inputs, plus 1e-6 x max |reference|.
The guide gradient jumps where luma * (L - 1) crosses an integer: pixels within 1e-4 of one are left out of the v_rgb
comparison only, at most 0.1 % of an input's pixels (asserted)."""
import ctypes
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import bilagrid_reference as R

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "host_math" / "bilagrid_host.cpp"
LIB = ROOT / "tests" / "host_math" / "libbilagrid_host.so"
HDR = ROOT / "3dgs-deblur_amd" / "csrc" / "bilagrid_math.h"
NEW_EXPORTS = {"gs_bilagrid_slice_fwd": 12, "gs_bilagrid_slice_bwd_workspace_bytes": 7, "gs_bilagrid_slice_bwd": 16,
               "gs_bilagrid_tv_workspace_bytes": 4, "gs_bilagrid_tv_fwd_bwd": 11}
SIZES = [(1, 1), (7, 5), (64, 48)]                  # (W, H)
SHAPES = [(16, 16, 8), (4, 6, 2), (2, 2, 2)]        # (GW, GH, L)


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def bh():
    if not LIB.exists() or LIB.stat().st_mtime < max(SRC.stat().st_mtime, HDR.stat().st_mtime):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", f"-I{HDR.parent}", str(SRC), "-o",
                               str(LIB)])
    lib = ctypes.CDLL(str(LIB))
    lib.bh_tv.restype = ctypes.c_double
    lib.bh_identity_channel.restype = ctypes.c_float
    return lib


def check_against_reference(got, grids, rgb, idx, v_out, what=""):
    """got = (out, v_rgb, v_grids) float32 tensors; the bound per output is measured, not chosen: 4 x the float32
    reference's own error + 1e-6 x max |float64 reference|; fragile pixels leave the v_rgb comparison only"""
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
        e_ours = (g.double() - r).abs()
        if mask is not None:
            e_torch, e_ours = e_torch[mask], e_ours[mask]
        bound = 4.0 * float(e_torch.max()) + 1e-6 * float(r.abs().max())
        print(f"{what} {name}: ours {float(e_ours.max()):.3e}, torch fp32 {float(e_torch.max()):.3e}, bound {bound:.3e}, "
              f"max|ref| {float(r.abs().max()):.3e}, fragile {n_frag}/{n_px}")
        assert float(e_ours.max()) <= bound, (what, name, float(e_ours.max()), bound)


def _host_slice(bh, grids, rgb, idx, v_out):
    B, H, W, _ = rgb.shape
    G, _, L, GH, GW = grids.shape
    gn, rn, vn = (np.ascontiguousarray(t.numpy()) for t in (grids, rgb, v_out))
    idn = np.asarray(idx, np.int32)
    out, v_rgb, v_grids = np.zeros_like(rn), np.zeros_like(rn), np.zeros_like(gn)
    bh.bh_slice_fwd(B, H, W, G, GW, GH, L, P(gn), P(idn), P(rn), P(out))
    bh.bh_slice_bwd(B, H, W, G, GW, GH, L, P(gn), P(idn), P(rn), P(vn), P(v_rgb), P(v_grids))
    return torch.from_numpy(out), torch.from_numpy(v_rgb), torch.from_numpy(v_grids)


# ---- host-compiled math ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("size", SIZES)
def test_header_math_against_the_grid_sample_reference(bh, size, shape):
    W, H = size
    seed = 100 + 10 * SIZES.index(size) + SHAPES.index(shape)
    for B, G, idx in ((1, 1, [0]), (3, 2, [1, 0, 1])):
        grids, rgb, v_out = R.random_case(B, H, W, G, shape, seed + B)
        luma = 0.299 * rgb[..., 0] + 0.587 * rgb[..., 1] + 0.114 * rgb[..., 2]
        if H * W >= 2:
            assert float(luma.min()) < 0 and float(luma.max()) > 1          # some guides leave [0, 1]
        got = _host_slice(bh, grids, rgb, idx, v_out)
        check_against_reference(got, grids, rgb, idx, v_out, what=f"host {W}x{H} {shape} B={B}")


def test_identity_grid_returns_the_input(bh, gs):
    grids = gs.bilagrid.identity_grids(1, (4, 6, 2))
    assert [bh.bh_identity_channel(c) for c in range(12)] == [float(v) for v in grids[0, :, 0, 0, 0]]
    _, rgb, v_out = R.random_case(1, 9, 11, 1, (4, 6, 2), 3)
    out, v_rgb, v_grids = _host_slice(bh, grids, rgb, [0], v_out)
    assert torch.allclose(out, rgb, atol=1e-6) and torch.allclose(v_rgb, v_out, atol=1e-6)
    assert float(v_grids.abs().max()) > 0


@pytest.mark.parametrize("shape", SHAPES)
def test_header_tv_against_the_sliced_reference(bh, shape):
    GW, GH, L = shape
    for G in (1, 3):
        grids, _, _ = R.random_case(1, 1, 1, G, shape, 7 + G)
        weight = 10.0
        gn = np.ascontiguousarray(grids.numpy())
        base = np.full_like(gn, 0.25)                                       # the gradient is ACCUMULATED
        v = base.copy()
        value = bh.bh_tv(G, GW, GH, L, P(gn), ctypes.c_float(weight), P(v))
        ref_v, ref_g = R.tv_ref_grads(grids, weight)
        ref32_v, ref32_g = R.tv_ref_grads(grids, weight, dtype=torch.float32)
        b_v = 4 * abs(float(ref32_v) - float(ref_v)) + 1e-6 * abs(float(ref_v))
        b_g = 4 * float((ref32_g.double() - ref_g).abs().max()) + 1e-6 * float(ref_g.abs().max())
        e_v = abs(value - float(ref_v))
        e_g = float((torch.from_numpy(v - base).double() - ref_g).abs().max())
        print(f"tv {shape} G={G}: value err {e_v:.3e} (bound {b_v:.3e}), grad err {e_g:.3e} (bound {b_g:.3e})")
        # subtracting the 0.25 the gradient was accumulated onto rounds at 0.25's precision: 2^-25 per element
        assert e_v <= b_v and e_g <= b_g + 2.0 ** -25


# ---- the torch restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("size", SIZES)
def test_torch_restatement_in_float64_agrees_with_the_reference(gs, size, shape):
    W, H = size
    grids, rgb, v_out = R.random_case(3, H, W, 2, shape, 50 + SIZES.index(size))
    idx = [1, 0, 1]
    g = grids.double().requires_grad_(True)
    r = rgb.double().requires_grad_(True)
    out = gs.bilagrid.slice(g, r, idx)
    v_rgb, v_grids = torch.autograd.grad(out, (r, g), v_out.double())
    ref = R.slice_ref_grads(grids, rgb, idx, v_out)
    frag = R.fragile_pixels(rgb, shape[2], eps=1e-9)[..., None].expand_as(rgb)
    assert int(frag.sum()) == 0
    assert float((out.detach() - ref[0]).abs().max()) <= 1e-10
    assert float((v_rgb - ref[1]).abs().max()) <= 1e-10
    assert float((v_grids - ref[2]).abs().max()) <= 1e-10
    t = gs.bilagrid.tv_loss(g, 10.0)
    (tg,) = torch.autograd.grad(t, g)
    rt, rg = R.tv_ref_grads(grids, 10.0)
    assert abs(float(t) - float(rt)) <= 1e-10 and float((tg - rg).abs().max()) <= 1e-10


def test_halves_and_single_image_form_agree_with_the_function(gs):
    grids, rgb, v_out = R.random_case(2, 12, 9, 3, (4, 6, 2), 21)
    idx = [2, 2]
    g = grids.clone().requires_grad_(True)
    r = rgb.clone().requires_grad_(True)
    out = gs.bilagrid.slice(g, r, idx)
    v_rgb, v_grids = torch.autograd.grad(out, (r, g), v_out)
    assert torch.equal(gs.bilagrid.slice_fwd(grids, rgb, idx), out.detach())
    h_rgb, h_grids = gs.bilagrid.slice_bwd(grids, rgb, idx, v_out)
    assert torch.equal(h_rgb, v_rgb) and torch.equal(h_grids, v_grids)
    assert float(h_grids[:2].abs().max()) == 0 and float(h_grids[2].abs().max()) > 0
    one = gs.bilagrid.slice(grids, rgb[1], 2)
    assert one.shape == rgb[1].shape and torch.allclose(one, out.detach()[1], atol=1e-6)
    # two images sharing a grid sum their gradients
    a = gs.bilagrid.slice_bwd(grids, rgb[0], 2, v_out[0])[1]
    b = gs.bilagrid.slice_bwd(grids, rgb[1], 2, v_out[1])[1]
    assert torch.allclose(a + b, h_grids, rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError):
        gs.bilagrid.slice(grids, rgb, [0, 3])
    with pytest.raises(ValueError):
        gs.bilagrid.slice(grids, rgb, [0])
    with pytest.raises(ValueError):
        gs.bilagrid.identity_grids(2, (16, 1, 8))


# ---- model surface ----------------------------------------------------------------------------------------------------
H_, W_ = 12, 16


def _model(gs, n=40, num_cameras=3, seed=0, **cfg_kw):
    g = torch.Generator().manual_seed(seed)
    cfg = gs.SplatfactoDeblurConfig(sh_degree=1, **cfg_kw)
    return gs.SplatfactoDeblurModel(cfg, torch.randn(n, 3, generator=g), torch.empty(n, 3).uniform_(-5.0, -3.0, generator=g),
                                    torch.randn(n, 4, generator=g), torch.empty(n).uniform_(0.0, 3.0, generator=g),
                                    torch.rand(n, 3, generator=g), torch.randn(n, 3, 3, generator=g) * 0.1,
                                    num_cameras=num_cameras)


def _stand_in_render(model, image=None):
    """replaces the HIP render below get_outputs (the host-logic tests' device): a fixed picture tinted by the parameters"""
    base = image if image is not None else torch.rand(H_, W_, 3, generator=torch.Generator().manual_seed(77)) * 0.8 + 0.1

    def fake_render(camera, detach_gaussians=False, return_depth=None):
        model.radii = torch.ones(1, model.num_points, dtype=torch.int32)
        tint = 0.01 * model.features_dc.mean(0)
        if model.pose_adjustment is not None:
            tint = tint + 0.1 * model.pose_adjustment[int(camera.metadata.get("cam_idx", 0))].sum()
        return {"rgb": base + tint[None, None, :]}
    model._render = fake_render
    return base


def _cam(gs, idx, H=H_, W=W_):
    md = {} if idx is None else {"cam_idx": idx}
    return gs.Camera(torch.eye(4)[:3], 10.0, 10.0, W / 2, H / 2, W, H, metadata=md)


def test_config_defaults_and_feature_off_builds_nothing(gs):
    c = gs.SplatfactoDeblurConfig()
    assert c.use_bilateral_grid is False and tuple(c.grid_shape) == (16, 16, 8) and c.bilateral_grid_tv_lambda == 10.0
    model = _model(gs)
    assert model.bilateral_grids is None
    assert "bilateral_grids" not in dict(model.named_parameters())
    assert set(gs.training.make_optimizers(model)) == {"means", "scales", "quats", "opacities", "features_dc",
                                                      "features_rest"}
    with pytest.raises(ValueError):
        model.get_outputs(_cam(gs, 0), bilateral_grid=True)


def test_feature_on_builds_identity_grids_and_their_optimizer(gs):
    model = _model(gs, num_cameras=5, use_bilateral_grid=True, grid_shape=(4, 6, 2))
    assert isinstance(model.bilateral_grids, torch.nn.Parameter) and model.bilateral_grids.shape == (5, 12, 2, 6, 4)
    assert torch.equal(model.bilateral_grids.detach(), gs.bilagrid.identity_grids(5, (4, 6, 2)))
    opts = gs.training.make_optimizers(model, lr_scale=0.5)
    assert set(opts) == {"means", "scales", "quats", "opacities", "features_dc", "features_rest", "bilateral_grid"}
    group = opts["bilateral_grid"].param_groups[0]
    assert group["lr"] == pytest.approx(1e-3) and group["eps"] == 1e-15 and group["params"][0] is model.bilateral_grids


def test_grid_is_applied_in_training_only_and_a_bad_cam_idx_raises(gs, monkeypatch):
    model = _model(gs, use_bilateral_grid=True, grid_shape=(4, 6, 2))
    base = _stand_in_render(model)
    with torch.no_grad():
        model.bilateral_grids[1, [0, 5, 10]] = 0.5                           # camera 1 halves every colour
    calls = []
    real = gs.bilagrid.slice
    monkeypatch.setattr(gs.bilagrid, "slice", lambda *a, **k: (calls.append(a[2]), real(*a, **k))[1])
    model.train()
    raw = base + 0.01 * model.features_dc.detach().mean(0)                    # what the stand-in renders
    assert torch.allclose(model.get_outputs(_cam(gs, 0))["rgb"].detach(), raw, atol=1e-6)      # identity grid
    assert torch.allclose(model.get_outputs(_cam(gs, 1))["rgb"].detach(), 0.5 * raw, atol=1e-6)
    assert calls == [0, 1]
    assert torch.equal(model.get_outputs(_cam(gs, 1), bilateral_grid=False)["rgb"].detach(), raw)
    assert torch.equal(model.get_outputs(_cam(gs, None))["rgb"].detach(), raw)   # a camera without an index
    model.eval()
    assert torch.equal(model.get_outputs(_cam(gs, 1))["rgb"].detach(), raw)
    assert torch.equal(model.get_outputs_for_camera(_cam(gs, 1))["rgb"], raw)
    assert torch.allclose(model.get_outputs(_cam(gs, 1), bilateral_grid=True)["rgb"].detach(), 0.5 * raw, atol=1e-6)
    assert len(calls) == 3
    model.train()
    rendered = []
    inner = model._render
    model._render = lambda *a, **k: (rendered.append(1), inner(*a, **k))[1]
    for bad in (3, -1):
        with pytest.raises(ValueError, match="cam_idx"):
            model.get_outputs(_cam(gs, bad))
        with pytest.raises(ValueError, match="cam_idx"):
            gs.training.train_step(model, gs.training.make_optimizers(model), _cam(gs, bad), base)
    assert not rendered                                                      # refused before anything was rendered


def test_eval_camera_step_renders_without_the_grid(gs, monkeypatch):
    cfg_kw = dict(use_bilateral_grid=True, grid_shape=(4, 6, 2))
    model = _model(gs, **cfg_kw)
    model.config.camera_optimizer.mode = "SO3xR3"
    model.pose_adjustment = torch.nn.Parameter(torch.zeros(3, 6))
    base = _stand_in_render(model)
    opts = gs.training.make_optimizers(model)
    calls = []
    real = gs.bilagrid.slice
    monkeypatch.setattr(gs.bilagrid, "slice", lambda *a, **k: (calls.append(a[2]), real(*a, **k))[1])
    loss = gs.training.eval_camera_step(model, opts, _cam(gs, 2), base * 0.9, ssim_lambda=0.0)
    assert loss == loss and not calls
    assert model.bilateral_grids.grad is None
    assert float(model.pose_adjustment.detach()[2].abs().sum()) > 0
    gs.training.train_step(model, opts, _cam(gs, 2), base * 0.9, ssim_lambda=0.0)
    assert calls == [2]


def test_train_step_reaches_the_grid_of_the_camera_and_adds_the_tv_term(gs):
    lam = 10.0
    model = _model(gs, use_bilateral_grid=True, grid_shape=(4, 6, 2), bilateral_grid_tv_lambda=lam)
    base = _stand_in_render(model)
    with torch.no_grad():
        model.bilateral_grids.add_(0.05 * torch.randn(model.bilateral_grids.shape, generator=torch.Generator().manual_seed(1)))
    start = model.bilateral_grids.detach().clone()
    gt = base * torch.tensor([0.8, 1.0, 1.2])
    opts = gs.training.make_optimizers(model)
    rgb = (base + 0.01 * model.features_dc.detach().mean(0)).double()[None]        # what the stand-in renders now
    h = gs.training.train_step(model, opts, _cam(gs, 1), gt, ssim_lambda=0.0)
    # the same loss and gradient from the float64 reference
    g = start.double().requires_grad_(True)
    l1 = (R.slice_ref(g, rgb, [1])[0] - gt.double()).abs().mean()
    total = l1 + lam * R.tv_ref(g)
    total.backward()
    assert h["loss"] == pytest.approx(float(total), rel=1e-5)
    assert torch.allclose(model.bilateral_grids.grad.double(), g.grad, rtol=1e-4, atol=1e-7)
    moved = (model.bilateral_grids.detach() != start).flatten(1).any(1)
    assert moved.tolist() == [True, True, True]       # the TV term reaches every grid; the image term grid 1 only
    corrected = R.slice_ref(start.double(), rgb, [1])[0]
    mse = float(((corrected.clamp(0, 1) - gt.double().clamp(0, 1)) ** 2).mean())
    assert h["psnr"] == pytest.approx(-10 * np.log10(mse), abs=1e-3)       # the PSNR of the CORRECTED image
    # the batch route: two views of one camera share a grid and sum their gradients
    model._render_batch = lambda cams, dg=False, rd=None: {"rgb": torch.stack([model._render(c)["rgb"] for c in cams])}
    start = model.bilateral_grids.detach().clone()
    rgb2 = (base + 0.01 * model.features_dc.detach().mean(0)).double()[None].expand(2, -1, -1, -1)
    gs.training.train_step(model, opts, [_cam(gs, 1), _cam(gs, 1)], [gt, gt * 0.9], ssim_lambda=0.0)
    g = start.double().requires_grad_(True)
    out = R.slice_ref(g, rgb2, [1, 1])
    tot = 0.5 * ((out[0] - gt.double()).abs().mean() + (out[1] - 0.9 * gt.double()).abs().mean()) + lam * R.tv_ref(g)
    tot.backward()
    assert torch.allclose(model.bilateral_grids.grad.double(), g.grad, rtol=1e-4, atol=1e-7)


def test_grid_only_fit_recovers_a_per_channel_gain_and_offset(gs):
    """a fixed 48 x 64 picture against itself x (0.8, 1.0, 1.2) + (0.02, -0.01, 0): only the grid can explain the
    difference.  train_step with its own optimizers (Adam 2e-3), L1 + TV; after 300 steps the L1 term is below one fifth
    of its initial value (on the grid_sample formulation it went 0.063 -> 0.0003)."""
    H, W = 48, 64
    model = _model(gs, num_cameras=1, use_bilateral_grid=True)
    g = torch.Generator().manual_seed(5)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    image = torch.stack([0.15 + 0.7 * xx, 0.2 + 0.6 * yy, 0.5 + 0.3 * torch.sin(6 * xx + 3 * yy)], dim=-1)
    image = (image + 0.02 * torch.randn(H, W, 3, generator=g)).clamp(0.02, 0.98)
    model._render = lambda camera, detach_gaussians=False, return_depth=None: {"rgb": image}
    gt = image * torch.tensor([0.8, 1.0, 1.2]) + torch.tensor([0.02, -0.01, 0.0])
    cam = _cam(gs, 0, H, W)
    opts = {"bilateral_grid": gs.training.make_optimizers(model)["bilateral_grid"]}

    def l1():
        model.train()
        with torch.no_grad():
            return float((model.get_outputs(cam)["rgb"] - gt).abs().mean())
    first = l1()
    for _ in range(300):
        gs.training.train_step(model, opts, cam, gt, ssim_lambda=0.0)
    last = l1()
    print(f"grid-only fit: L1 {first:.4f} -> {last:.5f}")
    assert first > 0.03 and last < first / 5.0, (first, last)


# ---- data parallel ------------------------------------------------------------------------------------------------
def _dp_worker(rank, world, port, q):
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    import gsdeblur_amd as gs
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    model = _model(gs, num_cameras=2, use_bilateral_grid=True, grid_shape=(4, 6, 2))
    base = _stand_in_render(model)
    opts = gs.training.make_optimizers(model)
    for step in range(3):
        i = (step + rank) % 2                               # the ranks see DIFFERENT views
        gt = base * torch.tensor([0.7 + 0.2 * i, 1.0, 1.1 + 0.1 * i])
        gs.training.train_step(model, opts, _cam(gs, i), gt, ssim_lambda=0.0, allreduce="sparse")
    flat = model.bilateral_grids.detach().reshape(-1).clone()
    other = [torch.zeros_like(flat) for _ in range(world)]
    dist.all_gather(other, flat)
    same = all(torch.equal(o, flat) for o in other)
    moved = [bool((model.bilateral_grids.detach()[k] != gs.bilagrid.identity_grids(1, (4, 6, 2))[0]).any()) for k in (0, 1)]
    q.put((rank, same, moved))
    dist.destroy_process_group()


def test_bilateral_grids_world2_gloo_stay_bit_identical():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 43300 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert res == [(0, True, [True, True]), (1, True, [True, True])]


# ---- C ABI ------------------------------------------------------------------------------------------------------
def _strip(txt):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


def test_new_exports_in_header_definitions_ctypes_table_and_integration_doc(gs):
    from gsdeblur_amd import _lib, _build
    hdr = _strip((ROOT / "include" / "gsdeblur.h").read_text())
    raw = (ROOT / "3dgs-deblur_amd" / "csrc" / "bilagrid.hip").read_text()
    src = _strip(raw)
    doc = (ROOT / "INTEGRATION.md").read_text()
    table = {**_lib._SIGS, **_lib._SIGS_LL}
    for name, nargs in NEW_EXPORTS.items():
        m = re.search(r"\b%s\s*\(([^;{}]*?)\)\s*;" % name, hdr)
        assert m, f"{name} not declared"
        assert len(m.group(1).split(",")) == nargs, name
        d = re.search(r"GS_EXPORT\s+[\w\s\*]+?\b%s\s*\(([^{};]*?)\)\s*\{" % name, src)
        assert d, f"{name} not defined in bilagrid.hip"
        assert len(d.group(1).split(",")) == nargs, name
        assert len(table[name]) == nargs and name in _lib.exported_names()
        assert hasattr(_lib.load(), name)
        assert f"`{name}`" in doc, f"{name} missing from INTEGRATION.md"
    assert "bilagrid.hip" in [s for s, _ in _build.SOURCES]
    # no environment, no allocation, no state, no float atomics in the new file
    for word in ("getenv", "hipMalloc", "hipFree", "static ", "atomicAdd", "atomic_add", "__hip_atomic"):
        assert word not in src, word
    lib = _lib.load()
    assert lib.gs_bilagrid_slice_bwd_workspace_bytes(0, 1080, 1920, 4, 16, 16, 8) == 0
    assert lib.gs_bilagrid_slice_bwd_workspace_bytes(1, 1080, 1920, 4, 16, 16, 8) > 0
    assert lib.gs_bilagrid_slice_bwd_workspace_bytes(1, 5, 7, 1, 16, 16, 8) > 0          # many cells under one tile
    assert lib.gs_bilagrid_slice_bwd_workspace_bytes(1, 0, 7, 1, 16, 16, 8) < 0
    assert lib.gs_bilagrid_slice_bwd_workspace_bytes(1, 5, 7, 1, 16, 1, 8) < 0
    assert lib.gs_bilagrid_tv_workspace_bytes(4, 16, 16, 8) > 0
    # B == 0 / G == 0 are no-ops that touch no pointer; invalid shapes are refused on the host
    assert lib.gs_bilagrid_slice_fwd(0, 4, 4, 1, 2, 2, 2, None, None, None, None, None) == 0
    assert lib.gs_bilagrid_slice_bwd(2, 4, 4, 0, 2, 2, 2, None, None, None, None, None, None, None, 0, None) == 0
    assert lib.gs_bilagrid_tv_fwd_bwd(0, 2, 2, 2, None, 1.0, None, None, None, 0, None) == 0
    assert lib.gs_bilagrid_slice_fwd(1, 4, 4, 1, 2, 1, 2, None, None, None, None, None) == 1
    assert lib.gs_bilagrid_slice_fwd(1, 4, 4, 1, 2, 2, 2, None, None, None, None, None) == 1      # null pointers


def test_hip_entry_points_refuse_cpu_tensors(gs):
    grids, rgb, v_out = R.random_case(1, 4, 4, 1, (2, 2, 2), 1)
    idx = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="no CPU fallback"):
        gs.bilagrid.slice_fwd_hip(grids, rgb, idx)
    with pytest.raises(ValueError, match="no CPU fallback"):
        gs.bilagrid.slice_bwd_hip(grids, rgb, idx, v_out)
    with pytest.raises(ValueError, match="no CPU fallback"):
        gs.bilagrid.tv_fwd_bwd_hip(grids, 1.0)
