"""TEST INFRASTRUCTURE (no tests here): the float64 yardstick of the depth-derived normals and their two losses
(3dgs-deblur_amd/normals.py, csrc/normals.hip), written with numpy from the statement of the op in csrc/normal_math.h, one
frame at a time, and the inputs the host and the GPU tests share.

reference(..., store=np.float32) rounds d, a, z, the rays, P, tx, ty, c, l2, n, m and g to float32 after every operation,
as the product does, and decides every mask on those values; store=None keeps float64 throughout (the masks then compare
float64 values against the same thresholds).  Sums, coefficients and gradients are float64 either way.  The difference of
the two is what float32 storage costs the reference itself: the tests' bound is 4 x that + 1e-6, for the loss as it is, for
the gradients and the normals relative to the frame's largest reference value (tolerances()); counts are exact.
"""
import numpy as np

MIN_L2 = np.float32(1e-30)
TERMS = {                      # the three ways the tests switch the terms on
    "prior": dict(use_prior=True, use_guide=False, prior_weight=0.7, smooth_weight=0.0, edge_beta=0.0),
    "smooth": dict(use_prior=False, use_guide=True, prior_weight=0.0, smooth_weight=0.4, edge_beta=2.0),
    "both": dict(use_prior=True, use_guide=True, prior_weight=0.7, smooth_weight=0.4, edge_beta=2.0),
}


def _pad(x):
    """one ring of zeros around the two leading axes"""
    return np.pad(x, [(1, 1), (1, 1)] + [(0, 0)] * (x.ndim - 2))


def _cross(a, b, t):
    return np.stack([(a[..., 1] * b[..., 2]).astype(t) - (a[..., 2] * b[..., 1]).astype(t),
                     (a[..., 2] * b[..., 0]).astype(t) - (a[..., 0] * b[..., 2]).astype(t),
                     (a[..., 0] * b[..., 1]).astype(t) - (a[..., 1] * b[..., 0]).astype(t)], axis=-1).astype(t)


def reference(depth_acc, alphas, intrins, prior=None, guide=None, prior_weight=1.0, smooth_weight=0.0, edge_beta=0.0,
              min_alpha=0.0, store=np.float32):
    """one frame: depth_acc, alphas [S,H,W], intrins fx fy cx cy, prior / guide [H,W,3] or None -> dict(loss, normals
    [H,W,3], defined, has_z [H,W], v_depth_acc, v_alphas [S,H,W] (float64), stats [6], min_l2: the smallest l2 of a defined
    normal)"""
    t = np.float64 if store is None else store
    acc, al = np.asarray(depth_acc).astype(t), np.asarray(alphas).astype(t)
    S, H, W = acc.shape
    d, a = acc[0], al[0]
    for s in range(1, S):
        d, a = (d + acc[s]).astype(t), (a + al[s]).astype(t)
    d, a = (d / t(S)).astype(t), (a / t(S)).astype(t)
    has = (a > t(np.float32(min_alpha))) & (d > 0)
    one = np.ones_like(d)
    z = (np.where(has, d, one) / np.where(has, a, one)).astype(t)
    fx, fy, cx, cy = (t(np.float32(k)) for k in intrins)
    rx = (((np.arange(W).astype(t) + t(0.5)).astype(t) - cx).astype(t) / fx).astype(t)[None, :]
    ry = (((np.arange(H).astype(t) + t(0.5)).astype(t) - cy).astype(t) / fy).astype(t)[:, None]
    P = _pad(np.stack([(rx * z).astype(t), (ry * z).astype(t), z], axis=-1).astype(t))
    hp = _pad(has)
    tx = (P[1:-1, 2:] - P[1:-1, :-2]).astype(t)
    ty = (P[2:, 1:-1] - P[:-2, 1:-1]).astype(t)
    c = _cross(ty, tx, t)
    l2 = (((c[..., 0] * c[..., 0]).astype(t) + (c[..., 1] * c[..., 1]).astype(t)).astype(t) + (c[..., 2] * c[..., 2]).astype(t)).astype(t)
    inner = np.zeros((H, W), bool)
    inner[1:-1, 1:-1] = True
    ok = inner & has & hp[1:-1, 2:] & hp[1:-1, :-2] & hp[2:, 1:-1] & hp[:-2, 1:-1]
    with np.errstate(invalid="ignore"):
        ok &= l2 > t(MIN_L2)
    root = np.sqrt(np.where(ok, l2, 1)).astype(t)
    n = np.where(ok[..., None], (c / root[..., None]).astype(t), 0).astype(t)
    defined = (n != 0).any(-1)
    n64 = n.astype(np.float64)
    pw, sw = float(np.float32(prior_weight)), float(np.float32(smooth_weight))
    # prior
    m64 = np.zeros((H, W, 3))
    use = np.zeros((H, W), bool)
    if prior is not None:
        p = np.asarray(prior, np.float32).astype(t)
        with np.errstate(invalid="ignore", over="ignore"):
            l = (((p[..., 0] * p[..., 0]).astype(t) + (p[..., 1] * p[..., 1]).astype(t)).astype(t) + (p[..., 2] * p[..., 2]).astype(t)).astype(t)
            has_m = (l > 0) & (l < np.inf)
        m = np.where(has_m[..., None], (np.where(has_m[..., None], p, 1) / np.sqrt(np.where(has_m, l, 1)).astype(t)[..., None]).astype(t), 0)
        use = has_m & defined
        m64 = np.where(use[..., None], m, 0).astype(np.float64)
    n_p = float(use.sum())
    s_p = float(np.where(use, 1.0 - (n64 * m64).sum(-1), 0.0).sum())
    # pairs: g[dy,dx] between a pixel and its neighbour at (+dy, +dx)
    np_, dp_ = _pad(n64), _pad(defined)
    gpad = None
    if guide is not None and edge_beta > 0:
        gpad = _pad(np.asarray(guide, np.float32).astype(t))
    pair_sum = np.zeros((H, W, 3))
    n_s = s_s = s_g = 0.0
    for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0)):
        sl = (slice(1 + dy, 1 + dy + H), slice(1 + dx, 1 + dx + W))
        both = defined & dp_[sl]
        if gpad is None:
            g = np.ones((H, W), t)
        else:
            diff = np.abs((gpad[1:-1, 1:-1] - gpad[sl]).astype(t))
            s = ((diff[..., 0] + diff[..., 1]).astype(t) + diff[..., 2]).astype(t)
            g = np.exp(-((t(np.float32(edge_beta)) * (s / t(3.0)).astype(t)).astype(t))).astype(t)
        g = np.where(both, g, 0).astype(np.float64)
        nq = np_[sl]
        pair_sum += g[..., None] * nq
        if dy + dx > 0:
            n_s += float(both.sum())
            s_s += float((g * np.where(both, 1.0 - (n64 * nq).sum(-1), 0.0)).sum())
            s_g += float(g.sum())
    kp = pw / n_p if n_p >= 1 else 0.0
    ks = sw / n_s if n_s >= 1 else 0.0
    loss = kp * s_p + ks * s_s
    vn = -kp * m64 - ks * pair_sum
    r64 = np.sqrt(np.where(defined, l2, 1).astype(np.float64))
    vc = np.where(defined[..., None], (vn - n64 * (n64 * vn).sum(-1, keepdims=True)) / r64[..., None], 0.0)
    vty = _pad(np.cross(tx.astype(np.float64), vc))
    vtx = _pad(np.cross(vc, ty.astype(np.float64)))
    vP = vtx[1:-1, :-2] - vtx[1:-1, 2:] + vty[:-2, 1:-1] - vty[2:, 1:-1]
    vz = rx.astype(np.float64) * vP[..., 0] + ry.astype(np.float64) * vP[..., 1] + vP[..., 2]
    d64, a64 = np.where(has, d, 1).astype(np.float64), np.where(has, a, 1).astype(np.float64)
    gd = np.where(has, vz / a64 / S, 0.0)
    ga = np.where(has, -(vz * d64) / (a64 * a64) / S, 0.0)
    shape = (S, H, W)
    return dict(loss=float(loss), normals=n64, defined=defined, has_z=has, v_depth_acc=np.broadcast_to(gd, shape).copy(),
                v_alphas=np.broadcast_to(ga, shape).copy(), min_l2=float(l2[defined].min()) if defined.any() else np.inf,
                stats=np.array([float(defined.sum()), n_p, s_p, n_s, s_s, s_g], np.float64))


def tolerances(depth_acc, alphas, intrins, **kw):
    """(reference(store=float32), loss tolerance, {v_depth_acc, v_alphas, normals: tolerance relative to the frame's largest
    reference value}): 4 x what float32 storage costs the reference itself, + 1e-6"""
    r32 = reference(depth_acc, alphas, intrins, store=np.float32, **kw)
    r64 = reference(depth_acc, alphas, intrins, store=None, **kw)
    assert np.array_equal(r32["defined"], r64["defined"]) and np.array_equal(r32["has_z"], r64["has_z"])
    assert np.array_equal(r32["stats"][[0, 1, 3]], r64["stats"][[0, 1, 3]])
    tol_loss = 4.0 * abs(r32["loss"] - r64["loss"]) + 1e-6
    tol = {}
    for k in ("v_depth_acc", "v_alphas", "normals"):
        top = np.abs(r64[k]).max() if r64[k].size else 0.0
        tol[k] = (4.0 * np.abs(r32[k] - r64[k]).max() / top if top > 0 else 0.0) + 1e-6
    return r32, tol_loss, tol


def check_frame(got_loss, got_v_depth_acc, got_v_alphas, got_normals, got_stats, depth_acc, alphas, intrins, what="", **kw):
    """assert one frame's results against the reference under the tolerance rule; -> the figures, for printing"""
    r32, tol_loss, tol = tolerances(depth_acc, alphas, intrins, **kw)
    err_loss = abs(float(got_loss) - r32["loss"])
    figures = {"loss": (err_loss, tol_loss)}
    assert err_loss <= tol_loss, (what, "loss", float(got_loss), r32["loss"], tol_loss)
    got_stats = np.asarray(got_stats, np.float64)
    assert np.array_equal(got_stats[[0, 1, 3]], r32["stats"][[0, 1, 3]]), (what, "counts", got_stats, r32["stats"])
    # float64 sums of non-negative terms (each within the rule of its reference term) in another order
    assert np.allclose(got_stats[[2, 4, 5]], r32["stats"][[2, 4, 5]], rtol=1e-5, atol=1e-6 * max(got_stats[0], 1.0)), (what, got_stats)
    degenerate = r32["stats"][1] * kw.get("prior_weight", 1.0) == 0 and r32["stats"][3] * kw.get("smooth_weight", 0.0) == 0
    if degenerate:
        assert float(got_loss) == 0.0, (what, "a frame without a term has loss", float(got_loss))
    for k, got in (("v_depth_acc", got_v_depth_acc), ("v_alphas", got_v_alphas), ("normals", got_normals)):
        if got is None:
            continue
        got = np.asarray(got, np.float64)
        assert got.shape == r32[k].shape, (what, k, got.shape)
        if k == "normals":
            assert np.array_equal((got != 0).any(-1), r32["defined"]), (what, "the normals' mask")
        else:
            dead = ~np.broadcast_to(r32["has_z"], got.shape) | degenerate
            assert not got[dead].any(), (what, k, "a pixel without z (or a degenerate frame) holds a non-zero gradient")
        top = np.abs(r32[k]).max() if got.size else 0.0
        err = (np.abs(got - r32[k]).max() / top if top > 0 else np.abs(got).max()) if got.size else 0.0
        figures[k] = (err, tol[k])
        assert err <= tol[k], (what, k, err, tol[k])
    return figures


# --------------------------------------------------------------------------- #
# inputs
# --------------------------------------------------------------------------- #
def intrinsics(H, W):
    return np.array([0.9 * W, 0.9 * W, 0.5 * W - 0.25, 0.5 * H + 0.125], np.float32)


def make_frame(S, H, W, seed, prior="noisy", alpha="covered"):
    """one frame of the prototype inputs: the bumpy surface 4 + 0.8 sin(x / 9) + 0.5 cos(y / 7) + 0.05 noise seen with
    fx = 0.9 W; per-sample alphas in [0.06, 1] with the depth sums alpha * depth (1 % per-sample noise); holes of alpha 0
    (depth sums exactly 0 there): single pixels, one in 40, and one block, in frames of at least 64 pixels; alpha="zero":
    alpha 0 everywhere.  Priors: vectors around (0, 0, -1) of length 0.5 .. 2.2, exactly zero at one pixel in nine;
    prior="none": zero everywhere.  The guide is a random image.
    -> float32 depth_acc [S,H,W], alphas [S,H,W], intrins [4], prior [H,W,3], guide [H,W,3]"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    depth = 4.0 + 0.8 * np.sin(x / 9.0) + 0.5 * np.cos(y / 7.0) + 0.05 * rng.standard_normal((H, W))
    covered = np.ones((H, W), bool)
    if H * W >= 64:
        covered &= rng.uniform(size=(H, W)) >= 1.0 / 40.0
        covered[H // 3:H // 3 + 3, W // 4:W // 4 + 4] = False
    if alpha == "zero":
        covered[:] = False
    else:
        assert alpha == "covered"
    al = rng.uniform(0.06, 1.0, (S, H, W)) * covered
    acc = al * depth * (1.0 + 0.01 * rng.standard_normal((S, H, W)))
    pr = np.stack([0.4 * rng.standard_normal((H, W)), 0.4 * rng.standard_normal((H, W)), -np.ones((H, W))], -1)
    pr *= rng.uniform(0.5, 2.0, (H, W, 1))
    if H * W > 9:
        pr[rng.uniform(size=(H, W)) < 1.0 / 9.0] = 0.0
    if prior == "none":
        pr[:] = 0.0
    else:
        assert prior == "noisy"
    guide = rng.uniform(size=(H, W, 3))
    return acc.astype(np.float32), al.astype(np.float32), intrinsics(H, W), pr.astype(np.float32), guide.astype(np.float32)


def make_batch(B, S, H, W, seed):
    """B frames; with B = 3 frame 1 has no prior value at all and frame 2 alpha 0 everywhere.  -> depth_acc, alphas
    [B,S,H,W], intrins [B,4], prior, guide [B,H,W,3]"""
    kinds = [("noisy", "covered"), ("none", "covered"), ("noisy", "zero")] if B == 3 else [("noisy", "covered")] * B
    frames = [make_frame(S, H, W, seed + 101 * b, *kinds[b]) for b in range(B)]
    return tuple(np.stack([f[k] for f in frames]) for k in range(5))


def assert_input_conditions(depth_acc, alphas, intrins, prior):
    """what makes the product's and the reference's masks identical, for every pixel: alphas exactly 0 or >= 0.05, d exactly
    0 where alpha is 0, priors exactly zero vectors or of length >= 0.5, every defined normal with l2 >= 1e-12 in both
    stores"""
    S = alphas.shape[0]
    assert ((alphas == 0) | (alphas >= 0.05)).all()
    d, a = depth_acc[0], alphas[0]
    for s in range(1, S):
        d, a = d + depth_acc[s], a + alphas[s]
    d, a = d / np.float32(S), a / np.float32(S)
    assert ((a == 0) | (a >= 0.05)).all() and (d[a == 0] == 0).all() and (d[a > 0] > 0).all()
    length = np.sqrt((prior.astype(np.float64) ** 2).sum(-1))
    assert ((length == 0) | (length >= 0.5)).all()
    for store in (np.float32, None):
        r = reference(depth_acc, alphas, intrins, store=store)
        assert r["min_l2"] >= 1e-12, (store, r["min_l2"])
