"""TEST INFRASTRUCTURE shared by tests/test_gpu_sh_degrees.py and tests/test_sh_degrees_host.py: the seeded scenes of the
(active SH degree, allocated coefficients K) cases and their float64 oracle frames, with the colour-clamp statistics.

The stock synthetic scenes draw DC at 0.5 randn and the rest at 0.05 randn: higher bands barely move the image and the
colour clamp max(SH + 0.5, 0) is reached by about none of the Gaussians.  Here DC is doubled and the rest multiplied by
6, so that every band carries signal and 4-16 % of the colours sit on the clamp."""
import math

import torch

# (active degree, allocated K): K > (deg + 1)^2 is the progressive schedule (model.active_sh_degree) or a caller's stride
CASES = [(0, 1), (0, 16), (1, 4), (1, 16), (2, 9), (2, 25), (3, 25), (4, 25)]
W, H, N, S, R = 128, 96, 2500, 3, 2
ET, RT, GAMMA, MLEVEL = 1 / 60, 1 / 30, 2.2, 10.0
BG = torch.tensor([0.05, 0.1, 0.15])
NAMES = ["means", "log_scales", "quats", "opacity_logits", "sh", "lin_vel", "ang_vel", "viewmat"]
CLAMP_BAND = 1e-5          # a pre-clamp colour this close to 0 (float64) may take the other side of the clamp in fp32
CLAMP_ROWS_MAX = 0.005     # share of the rows that may be left out of the sh comparison for that reason
CLAMPED_MIN = 0.02         # share of the colours on the clamp below which the clamp would not really be tested

# Share of fragile pixels (frame-level union over the sub-poses) the float64 ORACLE gives for each case's scene, measured
# on the CPU (tests/test_sh_degrees_host.py::test_recorded_oracle_shares re-derives two of them): a property of the
# seeded scene, not of the kernels.  The GPU tests hold each scene to 2x its share (test_gpu_parity.check_fragile).
FRAGILE_OBSERVED = {
    (0, 1): 0.01367, (0, 16): 0.01432, (1, 4): 0.01082, (1, 16): 0.01270,
    (2, 9): 0.01058, (2, 25): 0.01286, (3, 25): 0.01050, (4, 25): 0.01196,
}
FRAGILE_OBSERVED_PIXVEL = {(4, 25): 0.01229}
# measured with them: colours on the clamp 4.0 % (degree 0), 5.6-6.0 % (1), 8.6-8.9 % (2), 12.4 % (3), 16.2 % (4);
# colour-clamp-fragile rows: one, at (2,25) (smallest positive pre-clamp colour 4.3e-6), none elsewhere


def tag(deg, K, model="se3"):
    return f"sh deg={deg} K={K}" + ("" if model == "se3" else " pixvel")


def nb_of(deg):
    return (deg + 1) ** 2


def scene(O, deg, K, n=N):
    alloc = math.isqrt(K) - 1
    assert (alloc + 1) ** 2 == K and alloc >= deg
    sc = O.synthetic_scene(n, W, H, sh_degree=alloc, seed=330 + deg, scale_mult=5.0)
    sc["lin_vel"], sc["ang_vel"] = sc["lin_vel"] * 20, sc["ang_vel"] * 10        # visible motion at this size
    sc["opacity_logits"] = sc["opacity_logits"].clone()
    sc["opacity_logits"][::10] += 9.0                                            # the alpha clamp is reached
    sh = sc["sh"].clone()
    sh[:, 0] *= 2.0
    sh[:, 1:] *= 6.0
    sc["sh"] = sh
    return sc


def oracle_frame(O, sc, deg, model="se3", depth_fn=None, upstream=None):
    """the float64 frame of a case: -> dict with the leaves q, the config, image, per-sample images, fragile masks
    (frame level and per sample image), parts, the optional per-sample depth sums, and the colour-clamp statistics:
    clamped = share of (view, Gaussian, channel) colours on the clamp, clamp_rows = bool [N], Gaussians with a pre-clamp
    channel within CLAMP_BAND of 0 in a sub-pose where they are visible"""
    kw = {} if upstream is None else dict(upstream_grads=upstream)
    cfg = O.RenderConfig(H, W, sc["fx"], sc["fy"], sc["cx"], sc["cy"], sh_degree=deg, blur_samples=S, rs_bands=R,
                         exposure_time=ET, rolling_shutter_time=RT, gamma=GAMMA, min_rgb_level=MLEVEL,
                         motion_model=model, **kw)
    q = {k: sc[k].double().requires_grad_(True) for k in NAMES}
    ref, _, ref_samples, frag, parts, vms = O.render(
        cfg, q["means"], q["log_scales"].exp(), q["quats"], torch.sigmoid(q["opacity_logits"]), q["sh"], q["viewmat"],
        q["lin_vel"], q["ang_vel"], background=BG.double(), return_parts=True)
    _, samp_of, _ = O.subpose_times(S, ET, R, RT)
    frag_s = torch.zeros(S, H, W, dtype=torch.bool)
    for pi, part in enumerate(parts):
        frag_s[samp_of[pi]] |= part[4].fragile
    dref = None
    if depth_fn is not None:
        dref, dfrag = depth_fn(O, cfg, parts)
        frag = frag | dfrag               # (the depth composite shares the colour's thresholds: the same pixels)
    # colour statistics, from the pre-clamp colours of every view (the pixel-velocity model colours once, at mid exposure)
    with torch.no_grad():
        vis = torch.stack([part[0].radii > 0 for part in parts])                     # [P, N]
        pre = []
        for V in vms.detach():
            cam_pos = -(V[:3, :3].T @ V[:3, 3])
            pre.append(O.spherical_harmonics(deg, q["means"].detach() - cam_pos[None, :], q["sh"].detach()) + 0.5)
        pre = torch.stack(pre)                                                      # [P or 1, N, 3]
        if pre.shape[0] == 1:
            vis = vis.any(0, keepdim=True)
        clamped = float((pre <= 0).double().mean())
        clamp_rows = ((pre.abs() < CLAMP_BAND).any(-1) & vis).any(0)
        min_pos = float(pre[pre > 0].min())
    return dict(cfg=cfg, q=q, ref=ref, samples=ref_samples, frag=frag, frag_s=frag_s, parts=parts, depth=dref,
                clamped=clamped, clamp_rows=clamp_rows, min_pos=min_pos)


def loss_weights(frag, seed=5):
    """random pixel weights, zero on the fragile pixels (a flipped threshold there changes the gradient by O(1))"""
    return torch.rand(H, W, 3, generator=torch.Generator().manual_seed(seed)) * (~frag)[..., None]


def depth_weights(frag, seed=6):
    return (torch.rand(S, H, W, generator=torch.Generator().manual_seed(seed)) - 0.5) * 0.2 * (~frag)[None]
