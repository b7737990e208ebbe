"""The render path at GENERAL intrinsics (fx != fy, principal point off the centre, non-identity pose) and under the
exact symmetries of symmetry_cases.py.

Every other render comparison of the suite runs at fx == fy == 0.8 W, cx == W / 2, cy == H / 2, and compares HIP against
this repository's own restatement.  Here, for every configuration and every scene variant X (identity, mirror-x,
mirror-y with time reversed, transpose):
  (a) HIP(X) against the float64 oracle on X, at the project's own bars (IMG_ATOL, grad_el_ratio <= 1);
  (b) HIP(X) mapped back against HIP(identity): no reference VALUE is involved, only the oracle's fragile masks and, as
      the scale of the gradient bar, its identity-scene gradients.  Each side may sit one bar from the truth, hence
      2 * IMG_ATOL and grad_el_ratio <= 2 as reasoned; tightened to four times what was measured (REL_* below).
test_symmetry_host.py holds the oracle to the same relations at 1e-12, so a failure of (b) alone is a kernel's.
The relations are claimed at sizes that are multiples of the tile only; one ragged case goes through (a), and the model
surface is checked to hand its camera's four intrinsics through unchanged.
"""
import math

import numpy as np
import pytest
import torch

import symmetry_cases as SC
from absgrad_reference import frame_absgrad
from test_gpu_depth_grad import _oracle_depth
from test_gpu_parity import GRAD_EL_AFRAC, GRAD_EL_RTOL, IMG_ATOL, check_fragile, grad_el_ratio, rel_max

pytestmark = pytest.mark.gpu

DEPTH_RTOL = 2e-4              # rendered depth sums, of the frame's largest (test_depth_channel_of_the_sliced_path_...)
# relation (b): each side may sit one bar of (a) from the truth, so the bars reasoned beforehand are 2 * IMG_ATOL = 4e-4
# for image and alpha, a scaled grad_el_ratio of 2 for every gradient and statistic, 2 * DEPTH_RTOL for the depth image.
# Measured on the MI355X over all rows and variants (DESIGN.md §1 lists them per row): image / alpha 8.34e-7, gradients
# 0.113, depth 0.007 of its bar — each leaves far more than a factor of ten, so the bars are FOUR TIMES THE MEASURED
# worst value instead:
REL_IMG_ATOL = 3.4e-6          # 4 x 8.34e-7   (reasoned: 4e-4)
REL_GRAD_RATIO = 0.45          # 4 x 0.113     (reasoned: 2)
REL_DEPTH_RATIO = 0.03         # 4 x 0.007     (reasoned: 2), in units of DEPTH_RTOL * the frame's largest depth sum
assert REL_IMG_ATOL <= 2.0 * IMG_ATOL and REL_GRAD_RATIO <= 2.0 and REL_DEPTH_RATIO <= 2.0

SE3_S3 = SC.HOST_CONFIGS["se3 S=3"]
CONFIGS = {
    "1 se3 S=3": dict(cfg=SE3_S3),
    "2 se3 S=2 R=3, several slices": dict(cfg=SC.HOST_CONFIGS["se3 S=2 R=3"], slice_base=8),
    "3 pixvel S=3": dict(cfg=SC.HOST_CONFIGS["pixvel S=3"]),
    "4 pixvel exact-rs": dict(cfg=SC.HOST_CONFIGS["pixvel exact-rs S=2"]),
    "5 pixvel exact-rs shared list": dict(cfg=SC.HOST_CONFIGS["pixvel exact-rs shared S=2"]),
    "6 batch of two cameras, depth": dict(cfg=dict(blur_samples=2, rs_bands=1), batch=True),
    "7 se3 S=3, xy statistics": dict(cfg=SE3_S3, stats=True),
}
# the second camera of the batch: the first moved by this twist, its velocities scaled and reversed, a longer exposure
CAM2_SHIFT, CAM2_ROT, CAM2_VEL, CAM2_EXPOSURE = (-0.08, 0.05, 0.05), (-0.05, 0.08, -0.01), -1.2, 1.25 * SC.ET


def _cameras(O, sc, batch):
    """[(viewmat, lin_vel, ang_vel, exposure_time)] of the base scene, on the CPU"""
    cams = [(sc["viewmat"], sc["lin_vel"], sc["ang_vel"], SC.ET)]
    if batch:
        cams.append((SC.pose(O, sc["viewmat"], CAM2_SHIFT, CAM2_ROT), sc["lin_vel"] * CAM2_VEL, sc["ang_vel"] * CAM2_VEL,
                     CAM2_EXPOSURE))
    return cams


def _map_cameras(variant, cams):
    out = []
    for V, lin, ang, et in cams:
        d = SC.map_params(variant, dict(viewmat=V, lin_vel=lin, ang_vel=ang))
        out.append((d["viewmat"], d["lin_vel"], d["ang_vel"], et))
    return out


def _flat_grads(gauss, cams):
    """{name: gradient}: the Gaussians' and, per camera b, "viewmat[b]" (3 x 4 top), "lin_vel[b]", "ang_vel[b]" """
    out = dict(gauss)
    for b, c in enumerate(cams):
        for k in SC.CAM_NAMES:
            out[f"{k}[{b}]"] = c[k]
    return out


def _map_grads_back(variant, gauss, cams):
    return _flat_grads(SC.map_params(variant, gauss), [SC.map_params(variant, c) for c in cams])


# --------------------------------------------------------------------------- #
# the oracle on one scene variant
# --------------------------------------------------------------------------- #
def _oracle_forward(O, scX, camsX, case):
    """float64 frames of the cameras of a scene variant; fragile mask [B,H,W] (colour and depth passes)"""
    frames = []
    for V, lin, ang, et in camsX:
        f = SC.oracle_forward(O, scX, case["cfg"], camera=(V, lin, ang), exposure_time=et)
        if case.get("batch"):
            f["depth"], dfrag = _oracle_depth(O, f["cfg"], f["parts"])
            f["frag"] = f["frag"] | dfrag
        frames.append(f)
    return frames


def _oracle_backward(O, frames, case, wt, wd):
    """loss = sum_b img_b . wt_b (+ mean_s depth_b . wd_b) -> dict of [B,...] images and the flat gradients; with
    case['stats'] also the float64 signed / absolute screen-space centre sums"""
    loss = sum((f["img"] * wt[b]).sum() for b, f in enumerate(frames))
    if case.get("batch"):
        loss = loss + sum((f["depth"].mean(dim=0) * wd[b]).sum() for b, f in enumerate(frames))
    res = {}
    if case.get("stats"):
        f = frames[0]
        v_samples = torch.autograd.grad(loss, f["samples"], retain_graph=True)[0]
        res["xy"], res["xy_abs"] = frame_absgrad(O, f["cfg"], f["parts"], v_samples,
                                                 background=torch.tensor(SC.BACKGROUND, dtype=torch.float64))
    loss.backward()
    gauss = {k: sum(f["q"][k].grad for f in frames) for k in SC.G_NAMES}
    cams = [{k: (f["q"][k].grad[:3] if k == "viewmat" else f["q"][k].grad) for k in SC.CAM_NAMES} for f in frames]
    res.update(img=torch.stack([f["img"].detach() for f in frames]), alpha=torch.stack([f["alpha"].detach() for f in frames]),
               samples=[f["samples"].detach() for f in frames], gauss=gauss, cams=cams)
    if case.get("batch"):
        res["depth"] = torch.stack([f["depth"].detach().mean(dim=0) for f in frames])
    return res


# --------------------------------------------------------------------------- #
# the library on one scene variant
# --------------------------------------------------------------------------- #
def _hip(gs, dev, scX, camsX, case, wt, wd):
    """the same frame and loss through the HIP path -> the same dict as _oracle_backward, on the CPU in float64"""
    from gsdeblur_amd import ops
    kw_cfg = case["cfg"]
    S, R = int(kw_cfg["blur_samples"]), int(kw_cfg["rs_bands"])
    pixvel = kw_cfg.get("motion_model") == "pixel_velocity"
    exact, shared = bool(kw_cfg.get("rs_exact")), bool(kw_cfg.get("shared_list"))
    Hh, Ww, n = scX["height"], scX["width"], scX["means"].shape[0]
    p = {k: scX[k].float().to(dev).requires_grad_(True) for k in SC.G_NAMES}
    cp = [dict(zip(SC.CAM_NAMES, (t.float().to(dev).requires_grad_(True) for t in c[:3]))) for c in camsX]
    bg = torch.tensor(SC.BACKGROUND, device=dev)
    gargs = (p["means"], p["log_scales"].exp(), p["quats"], torch.sigmoid(p["opacity_logits"]), p["sh"])
    intr = (scX["fx"], scX["fy"], scX["cx"], scX["cy"], Hh, Ww)
    res = {}
    saved = ops.SLICE_BASE
    try:
        if case.get("slice_base"):
            ops.SLICE_BASE = case["slice_base"]
        if case.get("batch"):
            vms = torch.stack([gs.subpose_viewmats(c["viewmat"], c["lin_vel"], c["ang_vel"],
                                                   torch.tensor(gs.subpose_schedule(S, cam[3], R, SC.RT)[0], device=dev))
                               for c, cam in zip(cp, camsX)])
            rgb, alphas, _, dacc = gs.render_batch(*gargs, vms, bg, S, R, *intr, gamma=SC.GAMMA, min_rgb_level=SC.MLEVEL,
                                                   sh_degree=3, return_depth=True)
            img, alpha, depth = rgb, alphas.mean(dim=1), dacc.mean(dim=1)
            loss = (img * wt.float().to(dev)).sum() + (depth * wd.float().to(dev)).sum()
            res["depth"] = depth.detach().cpu().double()
        else:
            c = cp[0]
            kw = {}
            if case.get("stats"):
                kw = dict(xy_grad_out=torch.full((n, 2), 123.0, device=dev),
                          xy_absgrad_out=torch.full((n, 2), float("nan"), device=dev))
            if pixvel:
                times = gs.subpose_schedule(S, SC.ET, 1 if exact else R, 0.0 if exact else SC.RT)[0]
                vms = c["viewmat"]
                kw.update(lin_vel=c["lin_vel"], ang_vel=c["ang_vel"], rolling_shutter_time=SC.RT if exact else 0.0,
                          times=list(times) if shared else torch.tensor(times, device=dev), shared_list=shared)
            else:
                times = gs.subpose_schedule(S, SC.ET, R, SC.RT)[0]
                vms = gs.subpose_viewmats(c["viewmat"], c["lin_vel"], c["ang_vel"], torch.tensor(times, device=dev))
            samples, alphas, _ = gs.render_subposes(*gargs, vms, bg, S, R, *intr, sh_degree=3, **kw)
            out = gs.combine_samples(samples, SC.GAMMA, SC.MLEVEL)
            img, alpha = out[None], alphas.mean(dim=0)[None]
            loss = (img * wt.float().to(dev)).sum()
            res["samples"] = [samples.detach().cpu().double()]
        loss.backward()
        torch.cuda.synchronize()
        res["slices"] = sum(1 for v in ops.last_slice_intersects if int(v) > 0)
    finally:
        ops.SLICE_BASE = saved
    if case.get("stats"):
        res["xy"], res["xy_abs"] = kw["xy_grad_out"].cpu().double(), kw["xy_absgrad_out"].cpu().double()
    res.update(img=img.detach().cpu().double(), alpha=alpha.detach().cpu().double(),
               gauss={k: p[k].grad.cpu().double() for k in SC.G_NAMES},
               cams=[{k: (c[k].grad[:3] if k == "viewmat" else c[k].grad).cpu().double() for k in SC.CAM_NAMES} for c in cp])
    return res


def _scaled_ratio(a, b, scale):
    """grad_el_ratio of a against b with the tolerance taken from `scale` (the oracle's gradient): max over elements of
    |a - b| / (rtol |scale| + afrac max |scale|)"""
    a, b, scale = (np.asarray(t, np.float64) for t in (a, b, scale))
    tol = GRAD_EL_RTOL * np.abs(scale) + GRAD_EL_AFRAC * (np.abs(scale).max() + 1e-300)
    return float((np.abs(a - b) / tol).max())


@pytest.mark.parametrize("name", list(CONFIGS))
def test_general_intrinsics_vs_oracle_and_symmetry_relations(gs, oracle, dev, name):
    O = oracle
    case = CONFIGS[name]
    batch = bool(case.get("batch"))
    variants = SC.variants_of(case["cfg"])
    sc = SC.base_scene(O)
    cams = _cameras(O, sc, batch)
    B = len(cams)
    scenes = {X: SC.map_scene(X, sc) for X in variants}
    camsX = {X: _map_cameras(X, cams) for X in variants}
    # the oracle's fragile pixels of every variant, carried back to the base frame: the loss ignores their union on both
    # sides of (a) and (b), under the cap test_symmetry_host.py asserts for the oracle
    fwd = {X: _oracle_forward(O, scenes[X], camsX[X], case) for X in variants}
    frag = torch.zeros(B, SC.H, SC.W, dtype=torch.bool)
    for X in variants:
        fX = torch.stack([f["frag"] for f in fwd[X]])
        check_fragile(fX, f"symmetry {name} {X}")
        assert float(fX.double().mean()) <= SC.FRAGILE_CAP, (name, X)
        frag |= SC.map_image(X, fX, hdim=1)
    assert float(frag.double().mean()) <= SC.FRAGILE_CAP, name
    good = (~frag).double()
    wt = torch.stack([SC.loss_weights(seed=5 + b) for b in range(B)]) * good[..., None]                   # [B,H,W,3]
    wd = torch.stack([SC.loss_weights(seed=17 + b)[..., 0] for b in range(B)]) * good * 0.1               # [B,H,W]
    ora, hip = {}, {}
    for X in variants:
        wtX, wdX, goodX = (SC.map_image(X, t, hdim=1) for t in (wt, wd, good.bool()))
        ora[X] = _oracle_backward(O, fwd[X], case, wtX, wdX)
        hip[X] = _hip(gs, dev, scenes[X], camsX[X], case, wtX, wdX)
        if case.get("slice_base"):
            assert hip[X]["slices"] >= 2, (name, X, hip[X]["slices"])
        # ---- (a) HIP(X) against the oracle on X
        a_img = float((hip[X]["img"] - ora[X]["img"])[goodX].abs().max())
        a_alpha = float((hip[X]["alpha"] - ora[X]["alpha"])[goodX].abs().max())
        worst = {k: grad_el_ratio(g, _flat_grads(ora[X]["gauss"], ora[X]["cams"])[k])
                 for k, g in _flat_grads(hip[X]["gauss"], hip[X]["cams"]).items()}
        if "samples" in hip[X]:
            a_img = max(a_img, float((hip[X]["samples"][0] - ora[X]["samples"][0])[:, goodX[0]].abs().max()))
        if batch:
            worst["depth image / bar"] = float((hip[X]["depth"] - ora[X]["depth"])[goodX].abs().max()
                                               / (DEPTH_RTOL * float(ora[X]["depth"].max())))
        if case.get("stats"):
            worst["xy_grad_out"] = grad_el_ratio(hip[X]["xy"], ora[X]["xy"])
            worst["xy_absgrad_out"] = grad_el_ratio(hip[X]["xy_abs"], ora[X]["xy_abs"])
            assert float(ora[X]["xy_abs"].max()) > 0
        print(f"[symmetry (a) {name} | {X}] image {a_img:.2e} alpha {a_alpha:.2e} grad_el_ratio "
              + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
        assert a_img < IMG_ATOL and a_alpha < IMG_ATOL, (name, X, a_img, a_alpha)
        for k, v in worst.items():
            assert v <= 1.0, (name, X, k, v)
    # ---- (b) HIP(X) mapped back against HIP(identity); the oracle only lends its identity-scene gradients as the scale
    ident = hip["identity"]
    g_ident = _flat_grads(ident["gauss"], ident["cams"])
    g_scale = _flat_grads(ora["identity"]["gauss"], ora["identity"]["cams"])
    gb = good.bool()
    for X in variants[1:]:
        b_img = float((SC.map_image(X, hip[X]["img"], hdim=1) - ident["img"])[gb].abs().max())
        b_alpha = float((SC.map_image(X, hip[X]["alpha"], hdim=1) - ident["alpha"])[gb].abs().max())
        back = _map_grads_back(X, hip[X]["gauss"], hip[X]["cams"])
        worst = {k: _scaled_ratio(back[k], g_ident[k], g_scale[k]) for k in g_ident}
        b_depth = 0.0
        if batch:
            b_depth = float((SC.map_image(X, hip[X]["depth"], hdim=1) - ident["depth"])[gb].abs().max()
                            / (DEPTH_RTOL * float(ora["identity"]["depth"].max())))
        if case.get("stats"):
            worst["xy_grad_out"] = _scaled_ratio(SC.map_xy_grad(X, hip[X]["xy"]), ident["xy"], ora["identity"]["xy"])
            worst["xy_absgrad_out"] = _scaled_ratio(SC.map_xy_grad(X, hip[X]["xy_abs"], absolute=True), ident["xy_abs"],
                                                    ora["identity"]["xy_abs"])
        print(f"[symmetry (b) {name} | {X} vs identity] image {b_img:.2e} alpha {b_alpha:.2e} depth image / bar "
              f"{b_depth:.3f} scaled grad_el_ratio " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
        assert b_img < REL_IMG_ATOL and b_alpha < REL_IMG_ATOL, (name, X, b_img, b_alpha)
        assert b_depth <= REL_DEPTH_RATIO, (name, X, b_depth)
        for k, v in worst.items():
            assert v <= REL_GRAD_RATIO, (name, X, k, v)


# --------------------------------------------------------------------------- #
# a ragged size: (a) only — the relations are not claimed where the tile grid does not map onto itself
# --------------------------------------------------------------------------- #
RAGGED_W, RAGGED_H = 75, 45


def test_ragged_size_general_intrinsics_vs_oracle(gs, oracle, dev):
    O = oracle
    case = CONFIGS["1 se3 S=3"]
    sc = SC.base_scene(O, RAGGED_W, RAGGED_H)
    cams = _cameras(O, sc, False)
    fwd = _oracle_forward(O, sc, cams, case)
    frag = torch.stack([f["frag"] for f in fwd])
    check_fragile(frag, "symmetry ragged 75x45")
    assert float(frag.double().mean()) <= SC.FRAGILE_CAP
    good = ~frag
    wt = SC.loss_weights(RAGGED_H, RAGGED_W)[None] * good.double()[..., None]
    ora = _oracle_backward(O, fwd, case, wt, None)
    hip = _hip(gs, dev, sc, cams, case, wt, None)
    a_img = max(float((hip["img"] - ora["img"])[good].abs().max()),
                float((hip["samples"][0] - ora["samples"][0])[:, good[0]].abs().max()))
    a_alpha = float((hip["alpha"] - ora["alpha"])[good].abs().max())
    g_ora = _flat_grads(ora["gauss"], ora["cams"])
    worst = {k: grad_el_ratio(g, g_ora[k]) for k, g in _flat_grads(hip["gauss"], hip["cams"]).items()}
    print(f"[symmetry (a) ragged {RAGGED_W}x{RAGGED_H}] image {a_img:.2e} alpha {a_alpha:.2e} grad_el_ratio "
          + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert a_img < IMG_ATOL and a_alpha < IMG_ATOL, (a_img, a_alpha)
    for k, v in worst.items():
        assert v <= 1.0, (k, v)


def test_ragged_size_project_gaussians_parity(gs, oracle, dev):
    """the compat op at the ragged, off-centre, non-square camera, at the bars of test_project_gaussians_parity: integers
    and depth bits exact, xys / conics / cov3d bit-equal to the float32 oracle, compensation within 2 ulp, gradients
    against float64 autograd"""
    O = oracle
    W, H = RAGGED_W, RAGGED_H
    sc = SC.base_scene(O, W, H)
    n = sc["means"].shape[0]
    means = sc["means"].clone()
    means[:4, 2] = -1.0                        # behind the camera
    means[4:8, 0] *= 5.0                       # far off the screen
    V, scales, quats = sc["viewmat"], sc["log_scales"].exp(), sc["quats"] * 1.7
    intr = (sc["fx"], sc["fy"], sc["cx"], sc["cy"], H, W)
    pr = O.project_gaussians(means, scales, 1.0, quats, V, *intr)
    md, sd, qd, Vd = (t.to(dev).requires_grad_(True) for t in (means, scales, quats, V))
    xys, depths, radii, conics, comp, ntiles, cov3d = gs.project_gaussians(md, sd, 1.0, qd, Vd, *intr, 16)
    assert torch.equal(radii.cpu(), pr.radii)
    assert torch.equal(ntiles.cpu(), pr.num_tiles_hit)
    assert torch.equal(depths.cpu().view(torch.int32), pr.depths.view(torch.int32))
    ok = pr.radii > 0
    assert int(ok.sum()) > n // 2 and int((~ok).sum()) >= 4

    def ulps(a, b):
        return (a.cpu().contiguous().view(torch.int32).long() - b.contiguous().view(torch.int32).long()).abs()
    diag = {k: int(ulps(a[ok], b[ok]).max()) for k, (a, b) in dict(
        xys=(xys.detach(), pr.xys), conics=(conics.detach(), pr.conics), comp=(comp.detach(), pr.compensation),
        cov3d=(cov3d.detach(), pr.cov3d)).items()}
    print("[symmetry ragged project] float ulp diffs vs float32 oracle:", diag)
    assert diag["xys"] == 0 and diag["cov3d"] == 0 and diag["conics"] == 0, diag
    assert diag["comp"] <= 2, diag
    assert (xys.detach().cpu()[~ok] == 0).all()
    g = torch.Generator().manual_seed(1)
    vx, vd, vc, vcomp = (torch.randn(*s, generator=g) for s in ((n, 2), (n,), (n, 3), (n,)))
    loss = (xys * vx.to(dev)).sum() + (depths * vd.to(dev) * (radii > 0)).sum() + (conics * vc.to(dev)).sum() + \
        (comp * vcomp.to(dev)).sum()
    loss.backward()
    m64, s64, q64, V64 = (t.double().requires_grad_(True) for t in (means, scales, quats, V))
    prd = O.project_gaussians(m64, s64, 1.0, q64, V64, *intr)
    l64 = (prd.xys * vx.double()).sum() + (prd.depths * vd.double() * (prd.radii > 0)).sum() + \
        (prd.conics * vc.double()).sum() + (prd.compensation * vcomp.double()).sum()
    l64.backward()
    assert rel_max(md.grad.cpu(), m64.grad) < 3e-5
    assert rel_max(sd.grad.cpu(), s64.grad) < 3e-5
    assert rel_max(qd.grad.cpu(), q64.grad) < 3e-5
    assert rel_max(Vd.grad.cpu()[:3], V64.grad[:3]) < 3e-4


# --------------------------------------------------------------------------- #
# the model surface hands the camera's four intrinsics through
# --------------------------------------------------------------------------- #
def test_model_passes_general_intrinsics_through(gs, oracle, dev):
    """a gs.Camera with fx != fy and an off-centre principal point: get_outputs_for_camera == render_combined called with
    the camera's four values, render_normals == depth_normals with (fx, fy, cx, cy), fuse_tsdf == tsdf_integrate called
    directly — all bit for bit"""
    from gsdeblur_amd import ops
    from gsdeblur_amd.model import expected_depth
    sc = SC.base_scene(oracle)
    W, H = sc["width"], sc["height"]
    fx, fy, cx, cy = sc["fx"], sc["fy"], sc["cx"], sc["cy"]
    assert fx != fy and cx != W / 2 and cy != H / 2
    cfg = gs.SplatfactoDeblurConfig(blur_samples=2, rs_bands=3, gamma=SC.GAMMA, min_rgb_level=SC.MLEVEL)
    model = gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev)
    c2w = torch.linalg.inv(sc["viewmat"].double()).float()
    c2w[:3, 1] *= -1
    c2w[:3, 2] *= -1                           # OpenCV -> OpenGL camera axes
    lin, ang = sc["lin_vel"] * torch.tensor([1.0, -1.0, -1.0]), sc["ang_vel"] * torch.tensor([1.0, -1.0, -1.0])
    cam = gs.Camera(c2w[:3], fx, fy, cx, cy, W, H,
                    metadata=dict(camera_linear_velocity=lin.tolist(), camera_angular_velocity=ang.tolist(),
                                  exposure_time=SC.ET, rolling_shutter_time=SC.RT))

    def direct(S, R, times):
        viewmat, lv, av = model._viewmat_and_velocity(cam)
        vms = ops.subpose_viewmats(viewmat, lv, av, torch.tensor(times, dtype=torch.float32, device=dev))
        with torch.no_grad():
            rgb, alphas, _, dacc = gs.render_combined(
                model.means, model.scales, model.quats, model.opacities.reshape(-1), model.features_dc, vms,
                torch.zeros(3, device=dev), S, R, fx, fy, cx, cy, H, W, gamma=SC.GAMMA, min_rgb_level=SC.MLEVEL,
                sh_degree=3, return_depth=True, sh_rest=model.features_rest, raw_params=True)
        return torch.clamp(rgb, max=1.0), alphas.mean(dim=0)[..., None], expected_depth(dacc, alphas), viewmat

    out = model.get_outputs_for_camera(cam)
    rgb, acc, depth, viewmat = direct(2, 3, gs.subpose_schedule(2, SC.ET, 3, SC.RT)[0])
    assert float(rgb.max()) > 0.2 and float(acc.max()) > 0.9
    assert torch.equal(out["rgb"], rgb) and torch.equal(out["accumulation"], acc) and torch.equal(out["depth"], depth)
    # the sharp render (one sample, no bands) feeds the normals and the fusion
    rgb, acc, depth, viewmat = direct(1, 1, [0.0])
    sharp = model.sharp_outputs(cam)
    assert torch.equal(sharp["rgb"], rgb) and torch.equal(sharp["depth"], depth)
    m = (acc.reshape(1, H, W) > 0.5).float()
    normals = gs.depth_normals((depth.reshape(1, H, W) * m).contiguous(), m, (fx, fy, cx, cy))
    got = model.render_normals(cam)
    assert float(normals.abs().max()) > 0.5
    assert torch.equal(got, normals)
    lo, voxel, dims = (-1.5, -1.5, 0.5), 0.25, (13, 13, 41)
    fused = model.fuse_tsdf([cam], volume=gs.TSDFVolume(lo, voxel, dims, device=dev, color=True))
    ref = gs.TSDFVolume(lo, voxel, dims, device=dev, color=True)
    intrin = torch.tensor([[fx, fy, cx, cy]], dtype=torch.float32).to(dev)
    gs.tsdf_integrate(ref, depth.reshape(1, H, W).contiguous(), viewmat.detach().float()[None], intrin, 4.0 * voxel,
                      color=rgb.clamp(0.0, 1.0)[None], weights=(acc.reshape(1, H, W) >= 0.5).float(), depth_max=math.inf)
    assert float(ref.weight.sum()) > 0
    assert torch.equal(fused.tsdf, ref.tsdf) and torch.equal(fused.weight, ref.weight) and torch.equal(fused.color, ref.color)
