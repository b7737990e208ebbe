"""One table of small op cases for the stream-contract tests (tests/test_gpu_streams.py, tests/test_streams_host.py).

Every case is a function run(gs, dev) -> {name: tensor}: it builds its inputs from a fixed seed, calls the public op
(forward and, where there is one, backward) on whatever stream is current, and returns every output and gradient.  A case
never synchronises the device and never names a stream: the tests decide where it runs.  Builders and shapes are those of
the families' own GPU tests and reference modules (the smallest each of them uses that is more than a degenerate size).

`covers` lists the C-ABI symbols a case is meant to reach FROM PYTHON (the recording wrapper of the GPU test sees the calls
made through the ctypes object; what gs_frame_forward launches inside the library is covered by that symbol).  EXEMPT
names every entry point of include/gsdeblur.h that takes a stream and that no case covers, with the reason.

render_combined comes in three pieces (rc_prepare / rc_forward / rc_backward) so that the tests can interleave two
frames on two streams and can hand a frame inputs that only become right behind a delay on its own stream."""
import contextlib

import numpy as np
import torch

G_NAMES = ["means", "log_scales", "quats", "opacity_logits", "sh"]
CAM_NAMES = ["viewmat", "lin_vel", "ang_vel"]

CASES = []


class Case:
    def __init__(self, name, run, covers):
        self.name, self.run, self.covers = name, run, list(covers)

    def __repr__(self):
        return self.name


def case(name, covers):
    def deco(fn):
        CASES.append(Case(name, fn, covers))
        return fn
    return deco


def by_name(name):
    return next(c for c in CASES if c.name == name)


@contextlib.contextmanager
def ops_settings(**kw):
    """module switches of gsdeblur_amd.ops for the duration of a case, put back afterwards"""
    from gsdeblur_amd import ops
    old = {k: getattr(ops, k) for k in kw}
    try:
        for k, v in kw.items():
            setattr(ops, k, v)
        yield ops
    finally:
        for k, v in old.items():
            setattr(ops, k, v)


def _rand(shape, seed, dev, lo=-0.5, hi=0.5):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * (hi - lo) + lo).to(dev)


def _scene(gs, n=400, W=64, H=48, seed=41, deg=1, scale_mult=6.0):
    """the scene of the small batch / shutter tests: a few hundred Gaussians over 4 x 3 tiles, a moving camera"""
    sc = gs.data.synthetic_scene(n, W, H, sh_degree=deg, seed=seed, scale_mult=scale_mult)
    sc["lin_vel"], sc["ang_vel"] = sc["lin_vel"] * 20, sc["ang_vel"] * 10
    sc["W"], sc["H"], sc["deg"] = W, H, deg
    return sc


def _grads(d):
    return {f"grad_{k}": v.grad for k, v in d.items() if v.grad is not None}


def _camera_of_the_parity_test():
    import gs_oracle as O
    V0 = O.subpose_viewmats(torch.eye(4, dtype=torch.float64), torch.tensor([0.3, -0.2, 0.5], dtype=torch.float64),
                            torch.tensor([0.2, 0.4, -0.1], dtype=torch.float64), [1.0])[0].float()
    return V0, torch.tensor([0.1, 0.05, -0.2]), torch.tensor([0.05, -0.08, 0.03])


# ---- sub-pose view matrices -------------------------------------------------------------------------------------------------
def _subpose(gs, dev, with_times):
    V0, lin, ang = _camera_of_the_parity_test()
    P = 5
    times = torch.tensor([-0.02, -0.01, 0.0, 0.01, 0.3])
    go = torch.randn(P, 4, 4, generator=torch.Generator().manual_seed(P))
    go[:, 3, :] = 0
    Vd, ld, ad = (t.to(dev).requires_grad_(True) for t in (V0, lin, ang))
    td = times.to(dev).requires_grad_(with_times)
    out = gs.subpose_viewmats(Vd, ld, ad, td)
    (out * go.to(dev)).sum().backward()
    res = {"viewmats": out.detach(), "grad_viewmat": Vd.grad, "grad_lin": ld.grad, "grad_ang": ad.grad}
    if with_times:
        res["grad_times"] = td.grad
    return res


@case("subpose_viewmats_times", ["gs_subpose_viewmats_fwd", "gs_subpose_viewmats_bwd_times"])
def subpose_viewmats_times(gs, dev):
    return _subpose(gs, dev, True)


@case("subpose_viewmats", ["gs_subpose_viewmats_fwd", "gs_subpose_viewmats_bwd_store"])
def subpose_viewmats(gs, dev):
    return _subpose(gs, dev, False)


# ---- the three gsplat-style ops ---------------------------------------------------------------------------------------------
def _projected(gs, dev, sc, grad=False):
    V = _camera_of_the_parity_test()[0]
    leaves = [t.to(dev).requires_grad_(grad) for t in (sc["means"], sc["log_scales"].exp(), sc["quats"] * 1.7, V)]
    md, sd, qd, Vd = leaves
    out = gs.project_gaussians(md, sd, 1.0, qd, Vd, sc["fx"], sc["fy"], sc["cx"], sc["cy"], sc["H"], sc["W"], 16)
    return leaves, out


@case("project_gaussians", ["gs_project_fwd", "gs_project_bwd"])
def project_gaussians(gs, dev):
    sc = _scene(gs, seed=7, scale_mult=4.0)
    leaves, (xys, depths, radii, conics, comp, ntiles, cov3d) = _projected(gs, dev, sc, grad=True)
    loss = sum((t * _rand(t.shape, 20 + i, dev)).sum() for i, t in enumerate((xys, conics, comp, cov3d)))
    loss.backward()
    res = dict(xys=xys.detach(), depths=depths.detach(), radii=radii, conics=conics.detach(), comp=comp.detach(),
               ntiles=ntiles, cov3d=cov3d.detach())
    res.update(_grads(dict(zip(("means", "scales", "quats", "viewmat"), leaves))))
    return res


@case("spherical_harmonics", ["gs_sh_fwd", "gs_sh_bwd"])
def spherical_harmonics(gs, dev):
    g = torch.Generator().manual_seed(3)
    n, deg, K = 3000, 3, 16
    dirs = torch.randn(n, 3, generator=g) * 3.0
    cd = torch.randn(n, K, 3, generator=g).to(dev).requires_grad_(True)
    col = gs.spherical_harmonics(deg, dirs.to(dev), cd)
    (col * _rand(col.shape, 4, dev)).sum().backward()
    return {"colors": col.detach(), "grad_coeffs": cd.grad}


@case("rasterize_gaussians", ["gs_pack_records", "gs_rasterize_fwd", "gs_rasterize_bwd", "gs_unpack_record_grads",
                              "gs_make_depth_keys64", "gs_radix_sort_pairs_u64", "gs_radix_sort_pairs_u32",
                              "gs_exclusive_scan_u32", "gs_emit_intersects", "gs_tile_bin_edges_u32", "gs_gather_counts"])
def rasterize_gaussians(gs, dev):
    sc = _scene(gs, seed=17, scale_mult=4.0)
    n, H, W = sc["means"].shape[0], sc["H"], sc["W"]
    with torch.no_grad():
        _, (xys, depths, radii, conics, comp, ntiles, _) = _projected(gs, dev, sc)
    colors = torch.rand(n, 3, generator=torch.Generator().manual_seed(2))
    opac = torch.sigmoid(sc["opacity_logits"]).to(dev) * comp
    xd, cd, cold, od = (t.detach().to(dev).requires_grad_(True) for t in (xys, conics, colors, opac))
    bgd = torch.tensor([0.3, 0.6, 0.1]).to(dev).requires_grad_(True)
    img, alpha = gs.rasterize_gaussians(xd, depths, radii, cd, ntiles, cold, od[:, None], H, W, 16, bgd, return_alpha=True)
    ((img * _rand(img.shape, 5, dev)).sum() + (alpha * _rand(alpha.shape, 6, dev)).sum()).backward()
    res = {"img": img.detach(), "alpha": alpha.detach()}
    res.update(_grads(dict(xys=xd, conics=cd, colors=cold, opacity=od, background=bgd)))
    return res


@case("bin_and_sort_gaussians", ["gs_project_fwd", "gs_exclusive_scan_u32", "gs_map_gaussian_to_intersects", "gs_radix_sort_pairs_u64",
                                 "gs_tile_bin_edges_u64"])
def bin_and_sort_gaussians(gs, dev):
    sc = _scene(gs, seed=17, scale_mult=4.0)
    with torch.no_grad():
        _, (xys, depths, radii, conics, comp, ntiles, _) = _projected(gs, dev, sc)
    n_isect, cum = gs.compute_cumulative_intersects(ntiles)
    assert n_isect > 0
    tb = ((sc["W"] + 15) // 16, (sc["H"] + 15) // 16, 1)
    out = gs.bin_and_sort_gaussians(xys.shape[0], n_isect, xys, depths, radii, cum, tb)
    names = ("isect_ids", "gaussian_ids", "isect_ids_sorted", "gaussian_ids_sorted", "tile_bins")
    return dict(zip(names, (t[:n_isect] if i < 4 else t for i, t in enumerate(out))), cum=cum)


@case("gsplat_pixel_velocity", ["gs_project_pixvel_fwd", "gs_project_pixvel_bwd", "gs_sh_fwd", "gs_sh_bwd",
                                "gs_rasterize_fwd_rs_slice", "gs_rasterize_bwd_rs_slice", "gs_reduce_grad_tuples",
                                "gs_unpack_record_grads", "gs_combine_fwd", "gs_combine_bwd", "gs_make_depth_keys64",
                                "gs_radix_sort_pairs_u64", "gs_gather_counts", "gs_exclusive_scan_u32", "gs_emit_intersects",
                                "gs_radix_sort_pairs_carry_u32", "gs_tile_bin_edges_u32"])
def gsplat_pixel_velocity(gs, dev):
    """the fork-style keywords of project_gaussians / rasterize_gaussians, chained as the parity test chains them"""
    sc = _scene(gs, seed=80, deg=3)
    H, W, S, et, rt = sc["H"], sc["W"], 3, 1 / 60, 1 / 30
    bg = torch.tensor([0.05, 0.1, 0.15]).to(dev)
    p = {k: sc[k].float().to(dev).requires_grad_(True) for k in G_NAMES + CAM_NAMES}
    kw = dict(exposure_time=et, rolling_shutter_time=rt, blur_samples=S)
    qn = p["quats"] / p["quats"].norm(dim=-1, keepdim=True)
    xys, depths, radii, conics, comp, ntiles, cov3d, pv = gs.project_gaussians(
        p["means"], p["log_scales"].exp(), 1.0, qn, p["viewmat"], sc["fx"], sc["fy"], sc["cx"], sc["cy"], H, W,
        lin_vel=p["lin_vel"], ang_vel=p["ang_vel"], **kw)
    Vd = p["viewmat"].detach()
    cam = -(Vd[:3, :3].T @ Vd[:3, 3])
    rgb = torch.clamp(gs.spherical_harmonics(3, p["means"].detach() - cam[None, :], p["sh"]) + 0.5, min=0.0)
    op = torch.sigmoid(p["opacity_logits"]) * comp
    samples, alphas = gs.rasterize_gaussians(xys, depths, radii, conics, ntiles, rgb, op[:, None], H, W, 16, bg, True,
                                             pix_vels=pv, return_samples=True, **kw)
    out = gs.combine_samples(samples, 2.2, 10.0)
    (out * _rand(out.shape, 5, dev, 0.0, 1.0)).sum().backward()
    res = dict(samples=samples.detach(), alphas=alphas.detach(), out=out.detach(), radii=radii, ntiles=ntiles,
               pix_vels=pv.detach())
    res.update(_grads(p))
    return res


# ---- render_combined, SE(3): prepare / forward / backward -------------------------------------------------------------------
RC = dict(W=64, H=48, S=3, R=2, n=400)


def rc_inputs(gs, seed=41):
    """the CPU tensors a frame's leaves are made of (two seeds: two scenes of one shape with different values)"""
    sc = _scene(gs, RC["n"], RC["W"], RC["H"], seed=seed)
    return {k: sc[k].float() for k in G_NAMES + CAM_NAMES}, sc


def rc_prepare(gs, dev, seed=41):
    """everything of a frame that is uploaded (blocking copies): parameters, sub-pose times, loss weights"""
    cpu, sc = rc_inputs(gs, seed)
    S, R, H, W = RC["S"], RC["R"], RC["H"], RC["W"]
    return dict(sc=sc, params={k: v.to(dev) for k, v in cpu.items()},
                times=torch.tensor(gs.subpose_schedule(S, 1 / 60, R, 1 / 30)[0], device=dev),
                wc=_rand((H, W, 3), 7, dev) * (2.0 / (H * W)), wd=_rand((S, H, W), 17, dev) * (1.0 / (H * W)),
                wa=_rand((S, H, W), 27, dev) * (1.0 / (H * W)))


def rc_forward(gs, prep, lazy_select=True, depth=True, absgrad=True, learn_bg=False, pool=True, leaves=None):
    """the forward half; no host synchronisation before the frame call (tensor inputs only, all made by rc_prepare).
    leaves: device tensors to take as parameters instead of prep's (the backlog test fills them behind a delay)"""
    from gsdeblur_amd import ops
    sc, S, R, H, W = prep["sc"], RC["S"], RC["R"], RC["H"], RC["W"]
    src = prep["params"] if leaves is None else leaves
    p = {k: src[k].detach().requires_grad_(True) for k in G_NAMES + CAM_NAMES}
    dev = p["means"].device
    n = p["means"].shape[0]
    st = dict(p=p, prep=prep, depth=depth)
    st["xy"] = torch.zeros(n, 2, device=dev)
    st["xa"] = torch.zeros(n, 2, device=dev) if absgrad else None
    st["bg"] = torch.full((3,), 0.25, device=dev).requires_grad_(True) if learn_bg else None
    st["settings"] = dict(SLICE_BASE=2, LAZY_RECORDS=2 if lazy_select else 0, DEPTH_SELECT=2 if lazy_select else 0,
                          GRAD_POOL=bool(pool))
    with ops_settings(**st["settings"]):
        vms = gs.subpose_viewmats(p["viewmat"], p["lin_vel"], p["ang_vel"], prep["times"])
        out = gs.render_combined(p["means"], p["log_scales"].exp(), p["quats"], torch.sigmoid(p["opacity_logits"]),
                                 p["sh"], vms, st["bg"], S, R, sc["fx"], sc["fy"], sc["cx"], sc["cy"], H, W, gamma=2.2,
                                 min_rgb_level=10.0, sh_degree=sc["deg"], return_depth=depth, xy_grad_out=st["xy"],
                                 xy_absgrad_out=st["xa"], hints=ops.FrameHints())
        st["out"] = out
        st["slices"] = sum(1 for x in ops.last_slice_intersects if x > 0)
        st["depth_select"] = int(ops.last_depth_select)
    assert st["slices"] >= 2, f"the frame was meant to take several depth slices, it took {st['slices']}"
    return st


def rc_backward(st):
    prep, out, p = st["prep"], st["out"], st["p"]
    loss = (prep["wc"] * out[0]).sum() + (prep["wa"] * out[1]).sum()
    if st["depth"]:
        loss = loss + (prep["wd"] * out[3]).sum()
    with ops_settings(**st["settings"]):
        loss.backward()
    res = dict(rgb=out[0].detach(), alphas=out[1].detach(), radii=out[2], xy_grad=st["xy"],
               slices=torch.tensor(st["slices"]), depth_select=torch.tensor(st["depth_select"]))
    if st["depth"]:
        res["depth_acc"] = out[3].detach()
    if st["xa"] is not None:
        res["xy_absgrad"] = st["xa"]
    if st["bg"] is not None:
        res["grad_background"] = st["bg"].grad
    res.update(_grads(p))
    return res


_FRAME_FWD = ["gs_subpose_viewmats_fwd", "gs_project_fused_fwd", "gs_frame_forward"]


@case("render_combined_lazy_select", _FRAME_FWD + ["gs_frame_backward_depth", "gs_combine_bwd_scale", "gs_xy_absgrad_sum",
                                                   "gs_project_fused_bwd_pooled", "gs_subpose_viewmats_bwd_store"])
def render_combined_lazy_select(gs, dev):
    """lazy records and nearest-first selection forced on; depth gradient and absgrad"""
    res = rc_backward(rc_forward(gs, rc_prepare(gs, dev), lazy_select=True))
    assert int(res["depth_select"]) >= 1, "nearest-first selection did not run"
    return res


@case("render_combined_eager_full_sort", _FRAME_FWD + ["gs_frame_backward_depth", "gs_combine_bwd_scale",
                                                       "gs_xy_absgrad_sum", "gs_project_fused_bwd_pooled",
                                                       "gs_subpose_viewmats_bwd_store"])
def render_combined_eager_full_sort(gs, dev):
    """lazy records and nearest-first selection off; depth gradient and absgrad"""
    res = rc_backward(rc_forward(gs, rc_prepare(gs, dev), lazy_select=False))
    assert int(res["depth_select"]) == 0
    return res


@case("render_combined_background_unpooled", _FRAME_FWD + ["gs_frame_backward", "gs_combine_bwd", "gs_project_fused_bwd",
                                                           "gs_subpose_viewmats_bwd_store"])
def render_combined_background_unpooled(gs, dev):
    """a learnable background (two-step averaging backward), no depth channel, gradient buffers not pooled"""
    return rc_backward(rc_forward(gs, rc_prepare(gs, dev), lazy_select=True, depth=False, absgrad=False, learn_bg=True,
                                  pool=False))


# ---- render_subposes, pixel-velocity model ----------------------------------------------------------------------------------
@case("render_subposes_pixel_velocity", ["gs_project_pixvel_fwd", "gs_frame_forward", "gs_frame_backward",
                                         "gs_project_pixvel_bwd", "gs_combine_fwd", "gs_combine_bwd"])
def render_subposes_pixel_velocity(gs, dev):
    """exact rolling shutter with the shared list"""
    from gsdeblur_amd import ops
    sc = _scene(gs, seed=80, deg=3)
    H, W, S = sc["H"], sc["W"], 3
    p = {k: sc[k].float().to(dev).requires_grad_(True) for k in G_NAMES + CAM_NAMES}
    times, _, _ = gs.subpose_schedule(S, 1 / 60, 1, 0.0)
    samples, alphas, radii = gs.render_subposes(p["means"], p["log_scales"].exp(), p["quats"],
                                                torch.sigmoid(p["opacity_logits"]), p["sh"], p["viewmat"],
                                                torch.tensor([0.05, 0.1, 0.15]).to(dev), S, 1, sc["fx"], sc["fy"],
                                                sc["cx"], sc["cy"], H, W, sh_degree=3, lin_vel=p["lin_vel"],
                                                ang_vel=p["ang_vel"], times=torch.tensor(times, device=dev),
                                                rolling_shutter_time=1 / 30, shared_list=True, hints=ops.FrameHints())
    out = gs.combine_samples(samples, 2.2, 10.0)
    (out * _rand(out.shape, 5, dev, 0.0, 1.0)).sum().backward()
    res = dict(samples=samples.detach(), alphas=alphas.detach(), radii=radii, out=out.detach())
    res.update(_grads(p))
    return res


# ---- render_batch -----------------------------------------------------------------------------------------------------------
@case("render_batch", ["gs_subpose_viewmats_fwd", "gs_project_fused_fwd", "gs_frame_forward", "gs_frame_backward_depth",
                       "gs_frame_backward", "gs_combine_bwd_scale_batched", "gs_combine_bwd_batched",
                       "gs_project_fused_bwd_pooled", "gs_subpose_viewmats_bwd_store"])
def render_batch(gs, dev):
    """B = 2 cameras in one frame: once with a depth gradient and the per-camera xy statistic, once with a learnable
    background"""
    from gsdeblur_amd import ops
    sc = _scene(gs)
    H, W, S, R, B = sc["H"], sc["W"], 2, 2, 2
    n = sc["means"].shape[0]
    res = {}
    for tag, learn_bg in (("depth", False), ("bg", True)):
        p = {k: sc[k].float().to(dev).requires_grad_(True) for k in G_NAMES}
        cams, vms = [], []
        for b, (k, et) in enumerate(((1.0, 1 / 60), (-1.2, 1.25 / 60))):
            c = [sc["viewmat"].float().to(dev), (sc["lin_vel"].float() * k).to(dev), (sc["ang_vel"].float() * k).to(dev)]
            c = [t.requires_grad_(True) for t in c]
            cams.append(c)
            vms.append(gs.subpose_viewmats(*c, torch.tensor(gs.subpose_schedule(S, et, R, 1 / 30)[0], device=dev)))
        bg = torch.tensor([0.2, 0.5, 0.7]).to(dev).requires_grad_(True) if learn_bg else None
        xy = torch.zeros(B, n, 2, device=dev)
        rgb, al, radii, dacc = gs.render_batch(p["means"], p["log_scales"].exp(), p["quats"],
                                               torch.sigmoid(p["opacity_logits"]), p["sh"], torch.stack(vms), bg, S, R,
                                               sc["fx"], sc["fy"], sc["cx"], sc["cy"], H, W, gamma=2.2, min_rgb_level=10.0,
                                               sh_degree=sc["deg"], return_depth=True, xy_grad_out=xy,
                                               hints=ops.FrameHints())
        loss = (rgb * _rand(rgb.shape, 7, dev)).sum()
        if not learn_bg:
            loss = loss + (dacc * _rand(dacc.shape, 8, dev)).sum() * 0.1
        loss.backward()
        res.update({f"{tag}_rgb": rgb.detach(), f"{tag}_alphas": al.detach(), f"{tag}_radii": radii,
                    f"{tag}_depth_acc": dacc.detach(), f"{tag}_xy_grad": xy})
        res.update({f"{tag}_{k}": v for k, v in _grads(p).items()})
        for b in range(B):
            res.update({f"{tag}_cam{b}_{k}": v for k, v in _grads(dict(zip(CAM_NAMES, cams[b]))).items()})
        if learn_bg:
            res["bg_grad_background"] = bg.grad
    return res


# ---- render_step ------------------------------------------------------------------------------------------------------------
@case("render_step", ["gs_subpose_viewmats_fwd", "gs_project_fused_fwd", "gs_frame_forward", "gs_frame_backward",
                      "gs_combine_bwd_scale", "gs_project_fused_bwd_pooled", "gs_subpose_viewmats_bwd_times"])
def render_step(gs, dev):
    """the one-call route of the shutter test: raw parameters, features_dc + features_rest, the times gradient"""
    from gsdeblur_amd import ops
    W, H, S, R = 48, 32, 3, 2
    sc = _scene(gs, 300, W, H, seed=5)
    q = {k: sc[k].float().to(dev) for k in G_NAMES + CAM_NAMES}
    times = torch.tensor(gs.subpose_schedule(S, 1 / 30, R, 1 / 40)[0], device=dev)
    v_img = torch.randn(H, W, 3, generator=torch.Generator().manual_seed(9)).to(dev)
    dc, rest = q["sh"][:, 0, :].contiguous(), q["sh"][:, 1:, :].contiguous()
    rgb, g, radii = gs.render_step(q["means"], q["log_scales"], q["quats"], q["opacity_logits"], dc, q["viewmat"],
                                   q["lin_vel"], q["ang_vel"], times, None, S, R, sc["fx"], sc["fy"], sc["cx"], sc["cy"],
                                   H, W, v_img, gamma=2.2, min_rgb_level=10.0, sh_degree=1, sh_rest=rest, times_grad=True,
                                   hints=ops.FrameHints())
    res = {"rgb": rgb.detach().clone(), "radii": radii.clone()}
    res.update({f"grad_{k}": v.clone() for k, v in g.items() if v is not None})      # (views of a pooled buffer)
    return res


# ---- averaging --------------------------------------------------------------------------------------------------------------
@case("combine_samples", ["gs_combine_fwd", "gs_combine_bwd"])
def combine_samples(gs, dev):
    S, H, W = 3, 48, 64
    samples = _rand((S, H, W, 3), 11, dev, 0.0, 1.0).requires_grad_(True)
    out = gs.combine_samples(samples, 2.2, 10.0)
    (out * _rand(out.shape, 12, dev)).sum().backward()
    return {"out": out.detach(), "grad_samples": samples.grad}


# ---- training step ----------------------------------------------------------------------------------------------------------
@case("image_loss", ["gs_image_loss_fwd_bwd"])
def image_loss(gs, dev):
    from test_gpu_training import _images
    pred, gt = _images(37, 53, seed=5, flat=True)
    pg = pred.to(dev).requires_grad_(True)
    loss, parts = gs.fused.image_loss(pg, gt.to(dev), 0.2, return_parts=True)
    (3.0 * loss).backward()
    return {"loss": loss.detach(), "parts": parts.detach(), "grad_pred": pg.grad}


@case("hip_adam", ["gs_adam_step"])
def hip_adam(gs, dev):
    g = torch.Generator().manual_seed(5)
    shapes, lrs = [(3001, 3), (3001, 16, 3), (7, 6)], [1e-3, 2e-3, 1e-2]
    ps = [torch.nn.Parameter(torch.randn(s, generator=g).to(dev)) for s in shapes]
    opts = [gs.fused.HipAdam([p], lr=lr, eps=1e-15) for p, lr in zip(ps, lrs)]
    for _ in range(3):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g).to(dev)
        gs.fused.adam_step_all(opts)
    res = {}
    for i, (p, o) in enumerate(zip(ps, opts)):
        res.update({f"param{i}": p.detach(), f"exp_avg{i}": o.state[p]["exp_avg"], f"exp_avg_sq{i}": o.state[p]["exp_avg_sq"]})
    return res


@case("selective_adam", ["gs_adam_step_rows", "gs_adam_step", "gs_visible_rows"])
def selective_adam(gs, dev):
    """ten per-row tensors (two launches of gs_adam_step_rows) and one dense parameter under a row mask that comes from
    gs_visible_rows"""
    from gsdeblur_amd.fused import HipAdam, adam_step_all, visible_rows
    N = 3001
    g = torch.Generator().manual_seed(5)
    widths = [1, 3, 4, 45, 64, 3, 3, 1, 16, 2]
    ps = [torch.nn.Parameter(torch.randn(N, w, generator=g).to(dev)) for w in widths]
    cam = torch.nn.Parameter(torch.randn(7, 6, generator=g).to(dev))
    opts = [HipAdam([p], lr=1e-3 * (i + 1), eps=1e-15, selective=True) for i, p in enumerate(ps)]
    opts.append(HipAdam([cam], lr=1e-2, eps=1e-15))
    res = {}
    for step in range(2):
        radii = torch.randint(-2, 3, (6, N), generator=g, dtype=torch.int32)
        radii[radii == 1] = 0
        mask = visible_rows(radii.to(dev))
        for p in ps + [cam]:
            p.grad = torch.randn(p.shape, generator=g).to(dev)
        adam_step_all(opts, row_mask=mask)
        res[f"mask{step}"] = mask
    for i, (p, o) in enumerate(zip(ps + [cam], opts)):
        res.update({f"param{i}": p.detach(), f"exp_avg{i}": o.state[p]["exp_avg"]})
    return res


# ---- bilateral grid ---------------------------------------------------------------------------------------------------------
@case("bilagrid", ["gs_bilagrid_slice_fwd", "gs_bilagrid_slice_bwd", "gs_bilagrid_tv_fwd_bwd"])
def bilagrid(gs, dev):
    import bilagrid_reference as R
    grids, rgb, v_out = R.random_case(3, 48, 64, 3, (4, 6, 2), 324)
    gd, rd = grids.to(dev).requires_grad_(True), rgb.to(dev).requires_grad_(True)
    out = gs.bilagrid.slice(gd, rd, [2, 0, 2])
    (out * v_out.to(dev)).sum().backward()
    g2 = grids.to(dev).requires_grad_(True)
    tv = gs.bilagrid.tv_loss(g2, 0.5)
    tv.backward()
    return {"out": out.detach(), "grad_grids": gd.grad, "grad_rgb": rd.grad, "tv": tv.detach(), "grad_tv": g2.grad}


# ---- colour and scoring -----------------------------------------------------------------------------------------------------
@case("color_correct", ["gs_color_correct"])
def color_correct(gs, dev):
    import colorcorrect_reference as R
    k = R.case(3, 12, 16)
    out, warps = gs.color_correct(k["img"].to(dev), k["ref"].to(dev), return_warps=True)
    return {"out": out, "warps": warps}


@case("knn", ["gs_knn"])
def knn(gs, dev):
    """the clustered cloud: its five far outliers take the brute-force kernel"""
    import knn_reference as R
    d, i, stats = gs.knn(R.clustered().to(dev), 3, return_indices=True, return_stats=True)
    assert stats["fallback_rows"] >= 1, stats
    return {"dists": d, "idx": i, "fallback_rows": torch.tensor(int(stats["fallback_rows"]))}


@case("blur_stats", ["gs_blur_stats_ppt"])
def blur_stats(gs, dev):
    import blur_reference as R
    c = next(c for c in R.cases() if c["name"] == "F33")
    t = [torch.from_numpy(c[k]).to(dev) for k in ("points", "viewmats", "lin", "ang", "intrins", "times")]
    stats = gs.blur_stats(*t, c["W"], c["H"])
    return {"count": stats.count, **{k: getattr(stats, k) for k in R.STATS}}


# ---- geometry losses --------------------------------------------------------------------------------------------------------
@case("depth_prior", ["gs_depth_prior_loss"])
def depth_prior(gs, dev):
    import depthprior_reference as R
    acc, al, pr, _ = R.make_frame(5, 67, 131, "depth", seed=9)
    out = gs.depth_prior_loss_with_grad(torch.from_numpy(acc).to(dev), torch.from_numpy(al).to(dev),
                                        torch.from_numpy(pr).to(dev), "pearson", "depth", 0.7, 0.0, return_stats=True)
    return dict(zip(("loss", "grad_depth_acc", "grad_alphas", "stats"), out))


@case("normals", ["gs_depth_normals", "gs_normal_loss"])
def normals(gs, dev):
    import normal_reference as R
    acc, al, K, prior, guide = (np.ascontiguousarray(a) for a in R.make_frame(5, 67, 131, seed=209))
    f = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    out = gs.normal_loss_with_grad(f(acc), f(al), tuple(K.tolist()), f(prior), f(guide), prior_weight=0.7, smooth_weight=0.4,
                                   edge_beta=2.0, return_stats=True, return_normals=True)
    res = dict(zip(("loss", "grad_depth_acc", "grad_alphas", "stats", "normals"), out))
    res["depth_normals"] = gs.depth_normals(f(acc), f(al), tuple(K.tolist()))
    return res


# ---- TSDF -------------------------------------------------------------------------------------------------------------------
@case("tsdf_integrate", ["gs_tsdf_integrate"])
def tsdf_integrate(gs, dev):
    """frames_per_launch + 1 frames: two launches"""
    import tsdf_reference as R
    import test_tsdf_host as H
    assert H.K + 1 >= 17
    vol = H.torch_integrate(gs, dev, R.small_scene(H.K + 1), R.SMALL_TRUNC)
    return {"tsdf": vol.tsdf, "weight": vol.weight, "color": vol.color}


@case("tsdf_extract_mesh", ["gs_tsdf_mesh_count", "gs_tsdf_mesh_emit"])
def tsdf_extract_mesh(gs, dev):
    import tsdf_reference as R
    import test_tsdf_host as H
    f = R.sphere_field()
    vol = H.volume_of(gs, R.MESH_ORIGIN, 1.0, f, np.ones_like(f), R.field_colors(f.shape), device=dev)
    v, fc, c = gs.tsdf_extract_mesh(vol)
    assert len(v) > 0 and len(fc) > 0
    return {"verts": v, "faces": fc, "colors": c}


# ---- mesh clean-up ----------------------------------------------------------------------------------------------------------
def mesh_inputs(dev):
    import meshclean_reference as M
    V = 1025
    verts, colors = M.vertex_data(V)
    faces = M.edge_mesh(V, 1023)             # a strip over half the vertices, isolated triangles behind it
    return V, torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev), torch.from_numpy(colors).to(dev)


@case("mesh_clean", ["gs_mesh_components_round", "gs_mesh_components_finish", "gs_mesh_components_table",
                     "gs_mesh_filter_plan", "gs_mesh_filter_emit"])
def mesh_clean(gs, dev):
    V, verts, faces, colors = mesh_inputs(dev)
    labels, roots, fcount, vcount = gs.mesh_components(faces, V, return_table=True)
    v, f, c, stats = gs.mesh_filter_components(verts, faces, colors, min_faces=2, return_stats=True)
    assert stats["components"] > stats["kept"] >= 1, stats
    return dict(labels=labels, roots=roots, face_counts=fcount, vert_counts=vcount, verts=v, faces=f, colors=c,
                kept=torch.tensor(stats["kept"]))


# ---- MCMC -------------------------------------------------------------------------------------------------------------------
@case("mcmc", ["gs_mcmc_inject_noise", "gs_mcmc_relocation"])
def mcmc(gs, dev):
    from test_mcmc_host import noise_case, relocation_grid
    means, ls, q, l, _ = (t.to(dev) for t in noise_case(5000, seed=3))
    used = torch.empty(5000, 3, device=dev)
    gs.mcmc.inject_noise_hip(means, ls, q, l, 80.0, 7, 3, noise_out=used)
    o, s, n = (t.to(dev) for t in relocation_grid())
    new_o, new_s = gs.mcmc.relocation_hip(o, s, n)
    return {"means": means, "noise": used, "opacities": new_o, "scales": new_s}


# ---- data-parallel rows -----------------------------------------------------------------------------------------------------
DP_SHAPES = [(20011, 3), (20011, 3), (20011, 4), (20011, 1), (20011, 3), (20011, 15, 3)]


def dp_grads(dev, rank=0):
    g = torch.Generator().manual_seed(900 + rank)
    touched = torch.rand(DP_SHAPES[0][0], generator=g) < 0.03
    return [(torch.randn(s, generator=g) * touched.view(-1, *([1] * (len(s) - 1)))).to(dev) for s in DP_SHAPES]


def dp_exchange(row_ops, acc_ops):
    """row mask, pack, scatter and the masked-payload pair on two _RowOps (the sender's gradients, the receiver's)"""
    mask = row_ops.row_mask()
    idx = mask.nonzero().reshape(-1)
    M = idx.numel()
    assert M > 0
    pay = row_ops.pack(idx, M + 7)
    acc_ops.scatter_add(pay, M, 1.0 / 3)
    masked = row_ops.pack_masked(M + 5)
    acc_ops.scatter_add_payload(masked, M + 5, 0.5)
    res = {"mask": mask, "payload": pay, "masked_payload": masked}
    res.update({f"acc{i}": g for i, g in enumerate(acc_ops.grads)})
    return res


@case("dp_rows", ["gs_dp_row_mask", "gs_dp_pack_rows", "gs_dp_scatter_add_rows", "gs_dp_pack_masked_rows",
                  "gs_dp_scatter_add_payload"])
def dp_rows(gs, dev):
    from gsdeblur_amd.dp import _RowOps
    return dp_exchange(_RowOps(dp_grads(dev)), _RowOps([torch.zeros(s, device=dev) for s in DP_SHAPES]))


# ---- integer primitives -----------------------------------------------------------------------------------------------------
@case("integer_primitives", ["gs_exclusive_scan_u32", "gs_radix_sort_pairs_u32", "gs_radix_sort_pairs_u64",
                             "gs_radix_sort_pairs_carry_u32", "gs_radix_sort_pairs_gather_u32",
                             "gs_segmented_sort_pairs_u32"])
def integer_primitives(gs, dev):
    import python_frame_path
    g = torch.Generator().manual_seed(11)
    res = {}
    x = torch.randint(0, 300, (2049,), generator=g, dtype=torch.int32)
    res["scan"], res["scan_total"] = gs.exclusive_scan_u32(x.to(dev))
    n = 4097
    for name, bits, dtype in (("u32", 16, torch.int32), ("u64", 35, torch.int64)):
        keys = torch.randint(0, 2 ** bits, (n,), generator=g, dtype=torch.int64)
        keys[: n // 3] = keys[n // 3: 2 * (n // 3)]
        ks, vs = gs.radix_sort_pairs(keys.to(dtype).to(dev), torch.arange(n, dtype=torch.int32).to(dev), 0, bits)
        res[f"{name}_keys"], res[f"{name}_vals"] = ks[:n], vs[:n]
    keys = torch.randint(0, 2 ** 16, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    second = torch.randint(0, 2 ** 31 - 1, (n + 8,), generator=g, dtype=torch.int32).to(dev)
    ks, vs, ps = gs.radix_sort_pairs(keys.to(dev), None, 0, 16, carry=second)
    res["carry_keys"], res["carry_vals"], res["carry_payload"] = ks[:n], vs[:n], ps[:n]
    ks, vs, gt = gs.radix_sort_pairs(keys.to(dev), None, 0, 16, gather_src=second)
    res["gather_keys"], res["gather_vals"], res["gathered"] = ks[:n], vs[:n], gt[:n]
    P, N = 5, 4097
    keys = torch.randint(0, 2 ** 32, (P * N,), generator=g, dtype=torch.int64)
    keys[: N // 2] = keys[N // 2: 2 * (N // 2)]
    keys[-3:] = 0xFFFFFFFF
    ks, vs = python_frame_path.segmented_sort_pairs_u32(keys.to(torch.int32).to(dev), N)
    res["segmented_keys"], res["segmented_vals"] = ks[:P * N], vs[:P * N]
    return res


# ---- entry points no case covers --------------------------------------------------------------------------------------------
_INSIDE = ("launched by gs_frame_forward / gs_frame_backward inside the library on the frame's stream; from Python it is "
           "reached only by the legacy slice loop of tests/python_frame_path.py")
EXEMPT = {
    "gs_subpose_viewmats_bwd": "no caller in the package: the binding calls the _bwd_store and _bwd_times forms",
    "gs_blur_stats": "no caller in the package: blur_stats_hip always calls gs_blur_stats_ppt, the same kernels",
    "gs_rasterize_fwd_slice_stats": "debug twin of gs_rasterize_fwd_slice (lane statistics); " + _INSIDE,
    "gs_project_records": "no caller in the package (profiles/kernel_templates_refactor.md)",
    "gs_slice_project_records": "no caller in the package: the lazy-record projection is a step of gs_frame_forward",
    "gs_depth_select": "no caller in the package: a step of gs_frame_forward (nearest-first selection)",
    "gs_segmented_sort_select_u32": "no caller in the package: a step of gs_frame_forward (nearest-first selection)",
    "gs_slice_plan_select": "no caller in the package: a step of gs_frame_forward (nearest-first selection)",
    "gs_slice_counts_exact_swept": "no caller in the package: a step of gs_frame_forward (shared-list frames)",
    "gs_tile_bin_edges_ids_u32": "no caller in the package: a step of gs_frame_forward",
    "gs_combine_fwd_batched": "no caller in the package: gs_frame_forward launches the batched averaging itself",
    "gs_slice_colors": _INSIDE,
    "gs_segmented_sort_compact_u32": _INSIDE,
    "gs_exclusive_scan_segments_u32": _INSIDE,
    "gs_slice_plan": _INSIDE,
    "gs_tile_open_sat": _INSIDE,
    "gs_slice_counts": _INSIDE,
    "gs_slice_counts_exact": _INSIDE,
    "gs_emit_open_intersects": _INSIDE,
    "gs_rasterize_fwd_slice": _INSIDE,
    "gs_rasterize_bwd_slice": _INSIDE,
}
