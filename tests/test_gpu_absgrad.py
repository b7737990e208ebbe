"""Absgrad on the GPU: xy_absgrad_out of render_subposes / render_combined / render_batch / render_step against the
per-pair float64 reference (tests/absgrad_reference.py, anchored to the oracle in tests/test_absgrad_host.py); that asking
for it moves nothing else; determinism; batch rows; depth + absgrad in one call; untouched rows; training end to end.

Bar of the parity tests: the project's per-element gradient bar, grad_el_ratio <= 1, i.e. |d| <= 1e-4 |g| + 1e-5 max|g|.
The error of a sum of absolute values is bounded by the same sum of per-term errors as the signed sum, which meets this
bar on these scenes, and |g| and max|g| are no smaller."""
import math

import pytest
import torch

from absgrad_reference import frame_absgrad
from test_gpu_parity import grad_el_ratio
from test_gpu_depth_grad import _scene, _oracle_depth, NAMES

pytestmark = pytest.mark.gpu

MAX_FRAGILE_SHARE = 0.03          # of a frame's pixels, from the oracle alone


def _lib_frame(gs, dev, sc, S, R, H, W, combined, gamma, bg, want_xy=True, want_abs=True, depth=False, fill=None):
    """-> (params with requires_grad, colour output, depth_acc or None, xy_grad_out or None, xy_absgrad_out or None)"""
    p = {k: sc[k].to(dev).requires_grad_(True) for k in NAMES}
    times, _, _ = gs.subpose_schedule(S, 1 / 60, R, 1 / 30)
    vms = gs.subpose_viewmats(p["viewmat"], p["lin_vel"], p["ang_vel"], torch.tensor(times, device=dev))
    n = p["means"].shape[0]
    xy = torch.zeros(n, 2, device=dev) if want_xy else None
    xa = None
    if want_abs:
        xa = torch.empty(n, 2, device=dev)
        xa.fill_(float("nan") if fill is None else fill)
    args = (p["means"], p["log_scales"].exp(), p["quats"], torch.sigmoid(p["opacity_logits"]), p["sh"], vms,
            None if bg is None else bg.float().to(dev), S, R, sc["fx"], sc["fy"], sc["cx"], sc["cy"], H, W)
    kw = dict(xy_grad_out=xy, xy_absgrad_out=xa, return_depth=depth)
    if combined:
        res = gs.render_combined(*args, gamma=gamma, min_rgb_level=10.0, **kw)
    else:
        res = gs.render_subposes(*args, **kw)
    return p, res[0], (res[3] if depth else None), res[1], res[2], xy, xa


def _reference(O, sc, cfg, combined, bg, seed):
    """oracle frame + random upstream weights (zero on the fragile pixels) -> dict with the weights, the reference
    signed / absolute xy sums (float64 [N,2]) and the fragile share"""
    H, W = cfg.img_height, cfg.img_width
    q = {k: sc[k].double().requires_grad_(True) for k in NAMES}
    out, _, samples, frag, parts, _ = O.render(cfg, q["means"], q["log_scales"].exp(), q["quats"],
                                               torch.sigmoid(q["opacity_logits"]), q["sh"], q["viewmat"], q["lin_vel"],
                                               q["ang_vel"], background=bg, return_parts=True)
    per_part = max(float(pt[4].fragile.float().mean()) for pt in parts)
    share = float(frag.float().mean())
    print(f"fragile pixels: {share:.4%} of the frame, at most {per_part:.4%} per sub-pose")
    assert share <= MAX_FRAGILE_SHARE, share
    cref = out if combined else samples
    wc = torch.rand(cref.shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) - 0.5
    wc[..., frag, :] = 0.0
    wc = wc * (2.0 / (H * W))
    v_samples = torch.autograd.grad((wc * cref).sum(), samples, retain_graph=False)[0]
    sg, ab = frame_absgrad(O, cfg, parts, v_samples, background=bg)
    return dict(wc=wc, signed=sg, abs=ab, frag=frag)


def _reference_with_depth(O, sc, cfg, combined, seed):
    """as _reference, loss = wc . colour + wd . depth_acc.  Depth is a fourth colour with background 0: a pair's gradients
    of the two terms add BEFORE the absolute value, so the depth channel joins the colour dot product (colours [N,4],
    v [H,W,4] per sample)"""
    from absgrad_reference import absgrad_part
    H, W = cfg.img_height, cfg.img_width
    q = {k: sc[k].double().requires_grad_(True) for k in NAMES}
    out, _, samples, frag, parts, _ = O.render(cfg, q["means"], q["log_scales"].exp(), q["quats"],
                                               torch.sigmoid(q["opacity_logits"]), q["sh"], q["viewmat"], q["lin_vel"],
                                               q["ang_vel"], return_parts=True)
    dref, dfrag = _oracle_depth(O, cfg, parts)
    frag = frag | dfrag
    share = float(frag.float().mean())
    print(f"fragile pixels (colour and depth passes): {share:.4%} of the frame")
    assert share <= MAX_FRAGILE_SHARE, share
    wd = torch.rand(dref.shape, generator=torch.Generator().manual_seed(seed + 5), dtype=torch.float64) - 0.5
    wd[:, frag] = 0.0
    wd = wd / (H * W) * (1.0 / float(dref.detach().max()))       # the two terms of comparable size
    cref = out if combined else samples
    wc = torch.rand(cref.shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) - 0.5
    wc[..., frag, :] = 0.0
    wc = wc * (2.0 / (H * W))
    loss = (wc * cref).sum() + (wd * dref).sum()
    v_samples = torch.autograd.grad((wc * cref).sum(), samples, retain_graph=True)[0]
    loss.backward()
    _, samp, band = O.subpose_times(cfg.blur_samples, cfg.exposure_time, cfg.rs_bands, cfg.rolling_shutter_time)
    rows = O.band_tile_rows(H, cfg.rs_bands)
    sg = ab = 0.0
    for p, (pr, keys, gids, bins, r, rgb, op) in enumerate(parts):
        col4 = torch.cat([rgb.detach(), pr.depths.detach()[:, None]], dim=1)
        v4 = torch.cat([v_samples[samp[p]], wd[samp[p]][..., None]], dim=-1)
        s1, a1 = absgrad_part(O, pr.xys.detach(), pr.conics.detach(), col4, op.detach(), gids, bins, H, W, v4,
                              tile_rows=rows[band[p]], upstream=int(cfg.upstream_grads))
        sg, ab = sg + s1, ab + a1
    return dict(wc=wc, wd=wd, signed=sg, abs=ab, q=q)


CASES = [(1, 1, 0, False, None), (3, 2, 8, False, (0.3, 0.6, 0.1)), (5, 1, 0, True, None)]


@pytest.mark.parametrize("S,R,base,combined,bg", CASES)
def test_absgrad_matches_per_pair_reference(gs, oracle, dev, S, R, base, combined, bg):
    """measured on the MI355X (grad_el_ratio of absgrad / of xy_grad_out in the same call): see DESIGN.md"""
    from gsdeblur_amd import ops
    O = oracle
    W, H, n = 128, 96, 3000
    sc = _scene(O, n, W, H, 41)
    gamma = 2.2 if combined else 1.0
    bg_t = None if bg is None else torch.tensor(bg, dtype=torch.float64)
    cfg = O.RenderConfig(H, W, sc["fx"], sc["fy"], sc["cx"], sc["cy"], blur_samples=S, rs_bands=R, exposure_time=1 / 60,
                         rolling_shutter_time=1 / 30, gamma=gamma, min_rgb_level=10.0 if combined else 0.0)
    ref = _reference(O, sc, cfg, combined, bg_t, 7)
    old = ops.SLICE_BASE
    try:
        if base:
            ops.SLICE_BASE = base
        p, col, _, _, _, xy, xa = _lib_frame(gs, dev, sc, S, R, H, W, combined, gamma, bg_t)
        (ref["wc"].float().to(dev) * col).sum().backward()
        torch.cuda.synchronize()
        if base:
            assert sum(1 for x in ops.last_slice_intersects if x > 0) >= 2
    finally:
        ops.SLICE_BASE = old
    r_abs = grad_el_ratio(xa.cpu().numpy(), ref["abs"].numpy())
    r_sgn = grad_el_ratio(xy.cpu().numpy(), ref["signed"].numpy())
    touched = ref["abs"].norm(dim=-1) > 0
    med = float((ref["signed"].norm(dim=-1)[touched] / ref["abs"].norm(dim=-1)[touched]).median())
    print(f"S={S} R={R}: grad_el_ratio absgrad {r_abs:.3f}, signed {r_sgn:.3f}; median |signed| / absgrad {med:.3f}; "
          f"rows touched {int(touched.sum())}")
    assert float(ref["abs"].max()) > 0
    assert r_abs <= 1.0, r_abs
    assert r_sgn <= 1.0, r_sgn
    assert bool((xa >= xy.abs() * (1 - 1e-4) - 1e-5 * float(xa.max())).all())


def _all_outputs(gs, dev, sc, S, R, H, W, want_abs, depth, seed=3, want_xy=True):
    p, col, dacc, alphas, radii, xy, xa = _lib_frame(gs, dev, sc, S, R, H, W, True, 2.2, None, want_xy=want_xy,
                                                     want_abs=want_abs, depth=depth)
    g = torch.Generator().manual_seed(seed)
    loss = ((torch.rand(col.shape, generator=g) - 0.5).to(dev) * col).sum()
    loss = loss + ((torch.rand(alphas.shape, generator=g) - 0.5).to(dev) * alphas).sum() * 0.1
    if depth:
        loss = loss + ((torch.rand(dacc.shape, generator=g) - 0.5).to(dev) * dacc).sum() * 0.05
    loss.backward()
    torch.cuda.synchronize()
    out = {"rgb": col.detach(), "alphas": alphas.detach(), "radii": radii, "xy": xy}
    if depth:
        out["depth"] = dacc.detach()
    out.update({"g_" + k: v.grad for k, v in p.items()})
    return out, xa


@pytest.mark.parametrize("depth", [False, True])
@pytest.mark.parametrize("S,R,base", [(3, 1, 0), (3, 2, 8)])
def test_asking_for_absgrad_moves_nothing_else(gs, oracle, dev, depth, S, R, base):
    from gsdeblur_amd import ops
    W, H = 192, 128
    sc = _scene(oracle, 20000, W, H, 5)
    old = ops.SLICE_BASE
    try:
        if base:
            ops.SLICE_BASE = base
        a, _ = _all_outputs(gs, dev, sc, S, R, H, W, False, depth)
        b, xa = _all_outputs(gs, dev, sc, S, R, H, W, True, depth)
        c, xc = _all_outputs(gs, dev, sc, S, R, H, W, True, depth, want_xy=False)     # absgrad alone
    finally:
        ops.SLICE_BASE = old
    for k in a:
        assert a[k] is not None and torch.equal(a[k], b[k]), k
        if k != "xy":
            assert torch.equal(a[k], c[k]), k
    assert torch.equal(xa, xc) and float(xa.max()) > 0 and bool(torch.isfinite(xa).all())


def test_absgrad_is_deterministic(gs, oracle, dev):
    W, H = 192, 128
    sc = _scene(oracle, 20000, W, H, 6)
    runs = [_all_outputs(gs, dev, sc, 3, 2, H, W, True, False)[1].clone() for _ in range(3)]
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    assert float(runs[0].max()) > 0


def test_untouched_rows_are_zero_and_buffer_may_be_uninitialised(gs, oracle, dev):
    """the buffer arrives full of NaN; rows the frame never touched come back exactly zero.  Half of the Gaussians sit
    behind the camera, so such rows exist"""
    W, H, n = 128, 96, 4000
    sc = _scene(oracle, n, W, H, 9)
    sc["means"] = sc["means"].clone()
    Vm = sc["viewmat"].float()
    flip = torch.arange(n) % 2 == 0
    # mirror every other Gaussian through the camera centre: behind the camera, culled in every sub-pose
    centre = -(Vm[:3, :3].T @ Vm[:3, 3])
    sc["means"][flip] = (2 * centre[None] - sc["means"].float()[flip]).to(sc["means"].dtype)
    p, col, _, _, radii, xy, xa = _lib_frame(gs, dev, sc, 3, 1, H, W, True, 2.2, None)
    (col * (torch.rand(col.shape, generator=torch.Generator().manual_seed(1)) - 0.5).to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(xa).all())
    culled = (radii <= 0).all(dim=0)
    assert int(culled.sum()) >= n // 4
    assert float(xa[culled].abs().max()) == 0.0
    assert float(xa[~culled].max()) > 0
    assert bool((xa >= 0).all())
    # a row with a non-zero signed gradient has a non-zero absgrad, and vice versa no gradient at all means zero
    assert bool((~(xy.abs().sum(-1) > 0) | (xa.sum(-1) > 0)).all())


def test_batch_rows_equal_single_camera_absgrad(gs, dev):
    from test_gpu_batch import _scene as _bscene, _cameras, _viewmats, _gauss, _args
    W, H, S, R, B = 192, 128, 3, 2, 3
    sc = _bscene(gs, 20000, W, H, 13)
    cams = _cameras(gs, sc, B)
    g = torch.Generator().manual_seed(4)
    wts = [(torch.rand(H, W, 3, generator=g) - 0.5).to(dev) for _ in range(B)]
    n = sc["means"].shape[0]

    def run_batch(depth):
        p = _gauss(sc, dev, grad=True)
        vms = torch.stack([_viewmats(gs, c, S, R, dev) for c in cams])
        xy = torch.zeros(B, n, 2, device=dev)
        xa = torch.full((B, n, 2), float("nan"), device=dev)
        res = gs.render_batch(*_args(p), vms, None, S, R, sc["fx"], sc["fy"], sc["cx"], sc["cy"], H, W, gamma=2.2,
                              min_rgb_level=10.0, xy_grad_out=xy, xy_absgrad_out=xa, return_depth=depth)
        loss = sum((wts[b] * res[0][b]).sum() for b in range(B))
        if depth:
            loss = loss + sum((wts[b][..., 0] * res[3][b]).sum() for b in range(B)) * 0.05
        loss.backward()
        torch.cuda.synchronize()
        return xy, xa

    for depth in (False, True):
        xy, xa = run_batch(depth)
        for b in range(B):
            p = _gauss(sc, dev, grad=True)
            x1 = torch.zeros(n, 2, device=dev)
            a1 = torch.full((n, 2), float("nan"), device=dev)
            res = gs.render_combined(*_args(p), _viewmats(gs, cams[b], S, R, dev), None, S, R, sc["fx"], sc["fy"],
                                     sc["cx"], sc["cy"], H, W, gamma=2.2, min_rgb_level=10.0, xy_grad_out=x1,
                                     xy_absgrad_out=a1, return_depth=depth)
            loss = (wts[b] * res[0]).sum()
            if depth:
                loss = loss + (wts[b][..., 0] * res[3]).sum() * 0.05
            loss.backward()
            torch.cuda.synchronize()
            assert torch.equal(xa[b], a1), (depth, b)
            assert torch.equal(xy[b], x1), (depth, b)
            assert float(a1.max()) > 0


@pytest.mark.parametrize("depth", [False, True])
def test_batch_absgrad_in_several_slices_matches_per_pair_reference(gs, oracle, dev, depth):
    """a frame of two cameras (two samples each, 4 x 3 tiles) under a slice budget that forces several depth slices:
    raster_bwd_sload_kernel<true, 1, DEPTH, true, true>.  Every camera's absgrad and xy_grad_out rows against the
    per-pair reference of that camera alone, at the bar of test_absgrad_matches_per_pair_reference"""
    from gsdeblur_amd import ops
    from test_gpu_batch import _cameras, _viewmats, _args, G_NAMES
    O = oracle
    W, H, n, S, B = 64, 48, 400, 2, 2
    sc = _scene(O, n, W, H, 41)
    cams = _cameras(gs, sc, B, seed=1)
    refs = []
    for b, (V, lin, ang, et) in enumerate(cams):
        sc_b = dict(sc, viewmat=V, lin_vel=lin, ang_vel=ang)
        cfg = O.RenderConfig(H, W, sc["fx"], sc["fy"], sc["cx"], sc["cy"], blur_samples=S, rs_bands=1, exposure_time=et,
                             rolling_shutter_time=1 / 30, gamma=2.2, min_rgb_level=10.0)
        refs.append(_reference_with_depth(O, sc_b, cfg, True, 7 + b) if depth else _reference(O, sc_b, cfg, True, None, 7 + b))
    p = {k: sc[k].float().to(dev).requires_grad_(True) for k in G_NAMES}
    vms = torch.stack([_viewmats(gs, c, S, 1, dev) for c in cams])
    xy = torch.zeros(B, n, 2, device=dev)
    xa = torch.full((B, n, 2), float("nan"), device=dev)
    old = ops.SLICE_BASE
    try:
        ops.SLICE_BASE = 2
        res = gs.render_batch(*_args(p), vms, None, S, 1, sc["fx"], sc["fy"], sc["cx"], sc["cy"], H, W, gamma=2.2,
                              min_rgb_level=10.0, xy_grad_out=xy, xy_absgrad_out=xa, return_depth=depth)
        loss = sum((refs[b]["wc"].float().to(dev) * res[0][b]).sum() for b in range(B))
        if depth:
            loss = loss + sum((refs[b]["wd"].float().to(dev) * res[3][b]).sum() for b in range(B))
        loss.backward()
        torch.cuda.synchronize()
        assert sum(1 for x in ops.last_slice_intersects if x > 0) >= 2
    finally:
        ops.SLICE_BASE = old
    for b in range(B):
        r_abs = grad_el_ratio(xa[b].cpu().numpy(), refs[b]["abs"].numpy())
        r_sgn = grad_el_ratio(xy[b].cpu().numpy(), refs[b]["signed"].numpy())
        print(f"camera {b}, depth={depth}: grad_el_ratio absgrad {r_abs:.3f}, signed {r_sgn:.3f}")
        assert float(refs[b]["abs"].max()) > 0
        assert r_abs <= 1.0 and r_sgn <= 1.0, (b, r_abs, r_sgn)


@pytest.mark.parametrize("S,R,combined", [(1, 1, False), (5, 1, True)])
def test_depth_and_absgrad_in_one_call(gs, oracle, dev, S, R, combined):
    """return_depth=True with a depth loss term: absgrad (of the whole loss, the depth as a fourth colour), xy_grad_out
    and every parameter gradient meet their bars in the same call"""
    O = oracle
    W, H, n = 128, 96, 3000
    sc = _scene(O, n, W, H, 41)
    gamma = 2.2 if combined else 1.0
    cfg = O.RenderConfig(H, W, sc["fx"], sc["fy"], sc["cx"], sc["cy"], blur_samples=S, rs_bands=R, exposure_time=1 / 60,
                         rolling_shutter_time=1 / 30, gamma=gamma, min_rgb_level=10.0 if combined else 0.0)
    ref = _reference_with_depth(O, sc, cfg, combined, 7)
    p, col, dacc, _, _, xy, xa = _lib_frame(gs, dev, sc, S, R, H, W, combined, gamma, None, depth=True)
    ((ref["wc"].float().to(dev) * col).sum() + (ref["wd"].float().to(dev) * dacc).sum()).backward()
    torch.cuda.synchronize()
    r_abs = grad_el_ratio(xa.cpu().numpy(), ref["abs"].numpy())
    r_sgn = grad_el_ratio(xy.cpu().numpy(), ref["signed"].numpy())
    ratios = {}
    for k in NAMES:
        r, got = ref["q"][k].grad, p[k].grad.cpu()
        if k == "viewmat":
            r, got = r[:3], got[:3]
        if r is None or float(r.abs().max()) == 0.0:
            continue
        ratios[k] = grad_el_ratio(got.numpy(), r.numpy())
    print(f"depth + absgrad, S={S}: grad_el_ratio absgrad {r_abs:.3f}, signed {r_sgn:.3f}, parameters {ratios}")
    assert r_abs <= 1.0 and r_sgn <= 1.0, (r_abs, r_sgn)
    assert max(ratios.values()) <= 1.0, ratios


def test_render_step_fills_absgrad_like_the_autograd_route(gs, oracle, dev):
    from gsdeblur_amd.step import render_step
    W, H, S = 192, 128, 3
    sc = _scene(oracle, 20000, W, H, 5)
    times = torch.tensor(gs.subpose_schedule(S, 1 / 60, 1, 0.0)[0], device=dev, dtype=torch.float32)
    g_img = (torch.rand(H, W, 3, generator=torch.Generator().manual_seed(3)) - 0.5).to(dev)
    p = {k: sc[k].to(dev) for k in NAMES}
    n = p["means"].shape[0]
    xa = torch.full((n, 2), float("nan"), device=dev)
    render_step(p["means"], p["log_scales"], p["quats"], p["opacity_logits"], p["sh"], p["viewmat"], p["lin_vel"],
                p["ang_vel"], times, None, S, 1, sc["fx"], sc["fy"], sc["cx"], sc["cy"], H, W, g_img, gamma=2.2,
                min_rgb_level=10.0, raw_params=True, xy_absgrad_out=xa)
    vms = gs.subpose_viewmats(p["viewmat"], p["lin_vel"], p["ang_vel"], times)
    q = {k: p[k].clone().requires_grad_(True) for k in ("means", "log_scales", "quats", "opacity_logits", "sh")}
    xb = torch.full((n, 2), float("nan"), device=dev)
    rgb, _, _ = gs.render_combined(q["means"], q["log_scales"], q["quats"], q["opacity_logits"], q["sh"], vms, None, S, 1,
                                   sc["fx"], sc["fy"], sc["cx"], sc["cy"], H, W, gamma=2.2, min_rgb_level=10.0,
                                   raw_params=True, xy_absgrad_out=xb)
    (rgb * g_img).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(xa, xb) and float(xa.max()) > 0


@pytest.mark.timeout(1800)
def test_training_with_absgrad_densification_end_to_end(gs, dev, tmp_path):
    """the self-generated blurred dataset, densification driven by absgrad: at least two refinements run, the model grows,
    the loss falls, nothing is NaN.  (Whether it helps image quality is measured by tools/densify_e2e.py, not asserted.)"""
    import synthetic_dataset as SD
    from gsdeblur_amd import densify as D
    root = str(tmp_path / "ds")
    SD.generate(root, dev, width=160, height=112, n_frames=12, n_gaussians=4000, speed=1.0, dense_samples=16,
                seed_points=1000)
    scene = gs.load_transforms(root)
    images = gs.data.load_scene_images(scene, dev)
    xyz, rgb = gs.load_seed_points_ply(scene.ply_file_path)
    iters = 450
    dcfg = D.DensifyConfig(warmup_length=100, refine_every=100, reset_alpha_every=8, stop_split_at=iters,
                           stop_screen_size_at=200, absgrad=True)
    cfg = gs.SplatfactoDeblurConfig(sh_degree=3, blur_samples=5, gamma=2.2, min_rgb_level=0.0,
                                    rolling_shutter_compensation=False, use_scale_regularization=True,
                                    densify_absgrad=True)
    model = SD.init_from_seed_points(cfg, xyz, rgb, dev, num_cameras=len(scene.cameras))
    n0 = model.num_points
    r = gs.training.train_scene(model, scene, images, iters, densify=dcfg, log_every=1)
    losses = [float(h["loss"]) for h in r["history"]]
    assert len(losses) == iters and iters // dcfg.refine_every - 1 >= 2        # refinements at steps 200, 300, 400
    print("gaussians", n0, "->", model.num_points, "loss", sum(losses[:20]) / 20, "->", sum(losses[-20:]) / 20,
          "psnr", r["results"]["psnr"])
    assert all(math.isfinite(v) for v in losses)
    assert model.num_points > n0
    assert sum(losses[-20:]) / 20 < sum(losses[:20]) / 20
    for prm in model.gauss_params().values():
        assert bool(torch.isfinite(prm).all())
    # the switch without the model's statistic is an error, not a fallback
    cfg2 = gs.SplatfactoDeblurConfig(sh_degree=3, blur_samples=5, rolling_shutter_compensation=False)
    m2 = SD.init_from_seed_points(cfg2, xyz, rgb, dev, num_cameras=len(scene.cameras))
    with pytest.raises(ValueError, match="densify_absgrad"):
        gs.training.train_scene(m2, scene, images, 5, densify=dcfg)
