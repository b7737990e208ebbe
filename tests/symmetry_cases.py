"""Exact symmetries of the pinhole-plus-twist model: test infrastructure for test_symmetry_host.py / test_gpu_symmetry.py.

Every other render comparison of the suite runs at fx == fy == 0.8 W, cx == W / 2, cy == H / 2 and compares HIP against
this repository's own restatement.  The three maps below need no reference value: a scene X(scene) renders to X(image),
and its gradients map back to the scene's own, whoever computes them.  The base camera has fx != fy and an off-centre
principal point, so a swapped fx / fy or cx / cy, or a W / 2 written where cx belongs, breaks a relation.

  mirror_x            x -> -x: the image's columns flip
  mirror_y_reversed   y -> -y AND t -> -t: the rows flip, so does the readout order, hence both velocities are negated —
                      the relation that exercises the row bands and the exact per-row shutter
  transpose           x <-> y: the image transposes, W <-> H, fx <-> fy, cx <-> cy (frames without rolling shutter only)

Quaternions are (w, x, y, z); axial vectors (angular velocity, rotation axes) pick up the determinant -1 of the axis map.
W and H are multiples of the 16-pixel tile: a splat is cut at its tile box, so a pixel's value depends on the tile grid
and a map must carry the grid onto itself.  Two relations that look as natural do NOT hold and are not here: cropping by
whole tiles (the fov guard band 1.3 W / (2 fx) moves) and rotating the world (SH above degree 0 changes the colours).

Every parameter map is a signed permutation that is its own inverse, hence symmetric: the map that carries a parameter
to the variant scene also carries the variant's gradient back (map_params serves both directions).
"""
import math

import torch

W, H, N = 80, 48, 400
ET, RT, GAMMA, MLEVEL = 1 / 60, 1 / 30, 2.2, 10.0
BACKGROUND = (0.05, 0.1, 0.15)
G_NAMES = ["means", "log_scales", "quats", "opacity_logits", "sh"]
CAM_NAMES = ["viewmat", "lin_vel", "ang_vel"]
NAMES = G_NAMES + CAM_NAMES
VARIANTS = ("identity", "mirror_x", "mirror_y_reversed", "transpose")
FRAGILE_CAP = 0.005           # share of the pixels the oracle may flag in any configuration (measured: 0 .. 0.05 %)

# the oracle's RenderConfig keywords of the six configurations of the host test (sub-pose structure and motion model)
HOST_CONFIGS = {
    "se3 S=3": dict(blur_samples=3, rs_bands=1),
    "se3 S=2 R=3": dict(blur_samples=2, rs_bands=3),
    "pixvel S=3": dict(blur_samples=3, rs_bands=1, motion_model="pixel_velocity"),
    "pixvel S=2 R=3": dict(blur_samples=2, rs_bands=3, motion_model="pixel_velocity"),
    "pixvel exact-rs S=2": dict(blur_samples=2, rs_bands=1, motion_model="pixel_velocity", rs_exact=True),
    "pixvel exact-rs shared S=2": dict(blur_samples=2, rs_bands=1, motion_model="pixel_velocity", rs_exact=True,
                                       shared_list=True),
}


def has_rolling_shutter(cfg_kw):
    return int(cfg_kw.get("rs_bands", 1)) > 1 or bool(cfg_kw.get("rs_exact", False))


def variants_of(cfg_kw):
    """the scene variants whose relation holds for a configuration: the transpose needs a frame without rolling shutter"""
    return tuple(v for v in VARIANTS if not (v == "transpose" and has_rolling_shutter(cfg_kw)))


def pose(oracle, viewmat, shift, rot):
    """viewmat moved by a twist (the sub-pose map at t = 1), float64 on the CPU, returned as float32"""
    V = oracle.subpose_viewmats(viewmat.double(), torch.tensor(shift, dtype=torch.float64),
                                torch.tensor(rot, dtype=torch.float64), [1.0])[0]
    return V.float()


def base_scene(oracle, width=W, height=H, n=N):
    """the seeded scene at GENERAL intrinsics (fy = 1.37 fx, principal point off the centre by (9.3, -6.6)) and a
    non-identity pose: a 0.15 rad rotation about y plus a translation.  float32 tensors, as the library takes them"""
    sc = oracle.synthetic_scene(n, width, height, sh_degree=3, seed=7, scale_mult=4.0)
    sc["fx"] = 0.8 * width
    sc["fy"] = 1.37 * sc["fx"]
    sc["cx"] = width / 2 + 9.3
    sc["cy"] = height / 2 - 6.6
    c, s = math.cos(0.15), math.sin(0.15)
    V = torch.eye(4)
    V[:3, :3] = torch.tensor([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    V[:3, 3] = torch.tensor([0.1, -0.05, 0.2])
    sc["viewmat"] = V
    sc["lin_vel"], sc["ang_vel"] = sc["lin_vel"] * 20, sc["ang_vel"] * 10
    sc["exposure_time"], sc["rolling_shutter_time"] = ET, RT
    sc["width"], sc["height"] = width, height
    return sc


# --------------------------------------------------------------------------- #
# the maps
# --------------------------------------------------------------------------- #
_AXIS = {"mirror_x": ([0, 1, 2], [-1.0, 1.0, 1.0]), "mirror_y_reversed": ([0, 1, 2], [1.0, -1.0, 1.0]),
         "transpose": ([1, 0, 2], [1.0, 1.0, 1.0])}
_SH_NEGATE = {"mirror_x": [3, 4, 7, 10, 13, 15], "mirror_y_reversed": [1, 4, 5, 9, 10, 11]}


def _axis_map(variant, v):
    """the polar-vector map on the last dimension of v: M v (mirror) or P v (transpose)"""
    perm, sign = _AXIS[variant]
    return v[..., perm] * torch.tensor(sign, dtype=v.dtype, device=v.device)


def _map_sh(variant, sh):
    """SH coefficients [N,K,3] in the 3DGS order, up to degree 3 (K <= 16)"""
    K = sh.shape[1]
    assert K <= 16, "the SH maps are written out up to degree 3"
    out = sh.clone()
    if variant in _SH_NEGATE:
        idx = [k for k in _SH_NEGATE[variant] if k < K]
        out[:, idx] = -sh[:, idx]
        return out
    # x <-> y: swap 1 <-> 3, 5 <-> 7, 11 <-> 13; negate 8, 14; c9' = -c15, c15' = -c9
    for a, b, sgn in ((1, 3, 1.0), (5, 7, 1.0), (11, 13, 1.0), (9, 15, -1.0)):
        if b < K:
            out[:, a], out[:, b] = sgn * sh[:, b], sgn * sh[:, a]
    for k in (8, 14):
        if k < K:
            out[:, k] = -sh[:, k]
    return out


def map_params(variant, d):
    """{name: tensor} of scene parameters -> the variant scene's; of the variant's gradients -> the scene's own (every
    map is a symmetric involution).  Names outside NAMES pass through unchanged."""
    if variant == "identity":
        return dict(d)
    out = dict(d)
    reverse = variant == "mirror_y_reversed"
    for k, t in d.items():
        if k == "means":
            out[k] = _axis_map(variant, t)
        elif k == "log_scales":
            out[k] = t[:, [1, 0, 2]] if variant == "transpose" else t
        elif k == "quats":
            # rotation by theta about a -> about -(M a): the axis is axial
            out[k] = torch.cat([t[..., :1], -_axis_map(variant, t[..., 1:])], dim=-1)
        elif k == "sh":
            out[k] = _map_sh(variant, t)
        elif k == "viewmat":
            perm, sign = _AXIS[variant]
            A = torch.eye(4, dtype=t.dtype, device=t.device)[perm + [3]]
            A = A * torch.tensor(sign + [1.0], dtype=t.dtype, device=t.device)[:, None]
            out[k] = A[:t.shape[0], :t.shape[0]] @ t @ A.T          # [4,4], or the 3 x 4 top of a gradient
        elif k == "lin_vel":
            out[k] = _axis_map(variant, t) * (-1.0 if reverse else 1.0)
        elif k == "ang_vel":
            out[k] = -_axis_map(variant, t) * (-1.0 if reverse else 1.0)
    return out


def map_scene(variant, sc):
    """the variant scene of a base_scene dict: parameters, intrinsics and image size"""
    out = map_params(variant, sc)
    Wd, Ht = sc["width"], sc["height"]
    if variant == "mirror_x":
        out["cx"] = Wd - sc["cx"]
    elif variant == "mirror_y_reversed":
        out["cy"] = Ht - sc["cy"]
    elif variant == "transpose":
        out.update(fx=sc["fy"], fy=sc["fx"], cx=sc["cy"], cy=sc["cx"], width=Ht, height=Wd)
    return out


def map_image(variant, t, hdim=0):
    """an image-like tensor whose rows are dimension hdim and columns hdim + 1 (image [H,W,3], alpha / mask / weights
    [H,W], per-sample stacks [S,H,W] with hdim = 1) -> the variant's; its own inverse"""
    if variant == "identity":
        return t
    if variant == "mirror_x":
        return torch.flip(t, [hdim + 1])
    if variant == "mirror_y_reversed":
        return torch.flip(t, [hdim])
    return t.transpose(hdim, hdim + 1)


def map_xy_grad(variant, t, absolute=False):
    """the screen-space centre statistic [...,2] (xy_grad_out; absolute: xy_absgrad_out, which only swaps)"""
    if variant == "identity":
        return t
    if variant == "transpose":
        return t[..., [1, 0]]
    if absolute:
        return t
    sign = [-1.0, 1.0] if variant == "mirror_x" else [1.0, -1.0]
    return t * torch.tensor(sign, dtype=t.dtype, device=t.device)


# --------------------------------------------------------------------------- #
# the oracle on a scene
# --------------------------------------------------------------------------- #
def oracle_config(oracle, sc, cfg_kw, exposure_time=ET):
    return oracle.RenderConfig(sc["height"], sc["width"], sc["fx"], sc["fy"], sc["cx"], sc["cy"], exposure_time=exposure_time,
                               rolling_shutter_time=RT, gamma=GAMMA, min_rgb_level=MLEVEL, **cfg_kw)


def oracle_forward(oracle, sc, cfg_kw, camera=None, exposure_time=ET):
    """float64 oracle frame of a scene -> dict(cfg, q = leaf parameters, img, alpha, samples, frag, parts).
    camera: (viewmat, lin_vel, ang_vel) replacing the scene's own"""
    q = {k: sc[k].double().requires_grad_(True) for k in NAMES}
    if camera is not None:
        for k, t in zip(CAM_NAMES, camera):
            q[k] = t.double().requires_grad_(True)
    cfg = oracle_config(oracle, sc, cfg_kw, exposure_time)
    bg = torch.tensor(BACKGROUND, dtype=torch.float64)
    img, alpha, samples, frag, parts, _ = oracle.render(
        cfg, q["means"], q["log_scales"].exp(), q["quats"], torch.sigmoid(q["opacity_logits"]), q["sh"], q["viewmat"],
        q["lin_vel"], q["ang_vel"], background=bg, return_parts=True)
    return dict(cfg=cfg, q=q, img=img, alpha=alpha, samples=samples, frag=frag, parts=parts)


def grads_of(q):
    """{name: gradient} of the leaves of oracle_forward (the viewmat's as its 3 x 4 top)"""
    return {k: (q[k].grad[:3] if k == "viewmat" else q[k].grad).detach().clone() for k in NAMES}


def loss_weights(height=H, width=W, seed=5):
    """random loss weights [H,W,3] of the base frame, uniform in [0, 1); a variant's are map_image of these"""
    return torch.rand(height, width, 3, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def rel_to_max(a, b):
    """max |a - b| as a fraction of max |b|"""
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300))
