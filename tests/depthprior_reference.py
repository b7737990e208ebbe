"""TEST INFRASTRUCTURE (no tests here): the float64 yardstick of the depth-prior loss (3dgs-deblur_amd/depthprior.py,
csrc/depthprior.hip), written with numpy from the statement of the op in csrc/depthprior_math.h, one frame at a time, and
the inputs the host and the GPU tests share.

reference(..., store=np.float32) rounds d, a and x to float32 after every operation, as the product does, and decides
validity on those values; store=None keeps float64 throughout (validity then compares float64 values against the same
thresholds).  Sums, coefficients and gradients are float64 either way.  The difference of the two is what float32
storage costs the reference itself: the tests' bound is 4 x that + 1e-6, for the loss as it is, for the gradients
relative to the frame's largest reference gradient (tolerances()).
"""
import numpy as np

KINDS = ("pearson", "l1")
SPACES = ("depth", "disparity")
DEGENERATE_TOL = 1e-12


def reference(depth_acc, alphas, prior, kind="pearson", space="depth", weight=1.0, min_alpha=0.0, store=np.float32):
    """one frame: depth_acc, alphas [S,H,W], prior [H,W] -> dict(loss, v_depth_acc [S,H,W], v_alphas [S,H,W] (float64),
    valid [H,W], stats [8] = n, sx, sy, sxx, syy, sxy, sabs, rho, degenerate)"""
    assert kind in KINDS and space in SPACES
    t = np.float64 if store is None else store
    acc, al = np.asarray(depth_acc).astype(t), np.asarray(alphas).astype(t)
    S = acc.shape[0]
    d, a = acc[0], al[0]
    for s in range(1, S):
        d, a = (d + acc[s]).astype(t), (a + al[s]).astype(t)
    d, a = (d / t(S)).astype(t), (a / t(S)).astype(t)
    y32 = np.asarray(prior, np.float32)
    valid = (y32 > 0) & (a > t(np.float32(min_alpha)))
    if space == "disparity":
        valid &= d > 0
    one = np.ones_like(d)
    num, den = (d, a) if space == "depth" else (a, d)
    x = (np.where(valid, num, one) / np.where(valid, den, one)).astype(t)
    x = np.where(valid, x, 0).astype(np.float64)
    y = np.where(valid, y32, 0).astype(np.float64)
    w = float(np.float32(weight))
    n = float(valid.sum())
    sx, sy, sxx, syy, sxy = x.sum(), y.sum(), (x * x).sum(), (y * y).sum(), (x * y).sum()
    sabs = np.abs(x - y).sum() if kind == "l1" else 0.0
    rho = 0.0
    if kind == "l1":
        degenerate = n < 1
        loss = w * sabs / max(n, 1.0)
        g = np.sign(x - y) * (w / max(n, 1.0))
    else:
        vx, vy = n * sxx - sx * sx, n * syy - sy * sy
        degenerate = not (n >= 2 and vx > DEGENERATE_TOL * n * sxx and vy > DEGENERATE_TOL * n * syy)
        if degenerate:
            loss, g = 0.0, np.zeros_like(x)
        else:
            root = np.sqrt(vx * vy)
            rho = (n * sxy - sx * sy) / root
            loss = w * (1.0 - rho)
            g = -w * ((n * y - sy) / root - rho * (n * x - sx) / vx)
    live = valid & (not degenerate)
    d64, a64 = np.where(live, d, 1).astype(np.float64), np.where(live, a, 1).astype(np.float64)
    if space == "depth":
        gd, ga = g / a64, -(g * d64) / (a64 * a64)
    else:
        ga, gd = g / d64, -(g * a64) / (d64 * d64)
    gd, ga = np.where(live, gd / S, 0.0), np.where(live, ga / S, 0.0)
    shape = (S,) + d.shape
    return dict(loss=float(loss), v_depth_acc=np.broadcast_to(gd, shape).copy(), v_alphas=np.broadcast_to(ga, shape).copy(),
                valid=valid, degenerate=bool(degenerate),
                stats=np.array([n, sx, sy, sxx, syy, sxy, sabs, rho], np.float64))


def tolerances(depth_acc, alphas, prior, kind, space, weight=1.0, min_alpha=0.0):
    """(reference(store=float32), loss tolerance, gradient tolerance relative to the frame's largest reference gradient):
    4 x what float32 storage costs the reference itself, + 1e-6"""
    r32 = reference(depth_acc, alphas, prior, kind, space, weight, min_alpha, store=np.float32)
    r64 = reference(depth_acc, alphas, prior, kind, space, weight, min_alpha, store=None)
    assert np.array_equal(r32["valid"], r64["valid"]) and r32["degenerate"] == r64["degenerate"]
    tol_loss = 4.0 * abs(r32["loss"] - r64["loss"]) + 1e-6
    tol_grad = {}
    for k in ("v_depth_acc", "v_alphas"):
        top = np.abs(r64[k]).max()
        tol_grad[k] = (4.0 * np.abs(r32[k] - r64[k]).max() / top if top > 0 else 0.0) + 1e-6
    return r32, tol_loss, tol_grad


def check_frame(got_loss, got_v_depth_acc, got_v_alphas, depth_acc, alphas, prior, kind, space, weight=1.0, min_alpha=0.0,
                what=""):
    """assert one frame's results against the reference under the tolerance rule; -> the figures, for printing"""
    r32, tol_loss, tol_grad = tolerances(depth_acc, alphas, prior, kind, space, weight, min_alpha)
    err_loss = abs(float(got_loss) - r32["loss"])
    figures = {"loss": (err_loss, tol_loss)}
    assert err_loss <= tol_loss, (what, "loss", float(got_loss), r32["loss"], tol_loss)
    for k, got in (("v_depth_acc", got_v_depth_acc), ("v_alphas", got_v_alphas)):
        got = np.asarray(got, np.float64)
        assert got.shape == r32[k].shape, (what, k, got.shape)
        dead = ~np.broadcast_to(r32["valid"], got.shape) | r32["degenerate"]
        assert not got[dead].any(), (what, k, "an invalid pixel (or a degenerate frame) holds a non-zero gradient")
        top = np.abs(r32[k]).max()
        err = np.abs(got - r32[k]).max() / top if top > 0 else np.abs(got).max()
        figures[k] = (err, tol_grad[k])
        assert err <= tol_grad[k], (what, k, err, tol_grad[k])
    return figures


# --------------------------------------------------------------------------- #
# inputs
# --------------------------------------------------------------------------- #
def make_frame(S, H, W, space, seed, prior="noisy"):
    """one frame of the prototype inputs: depth in [2, 8], an eighth of the pixels uncovered (alphas and depth_acc exactly
    0 in every sample), the others with per-sample alphas in [0.06, 1] and 5 % per-sample noise on the depth sums; the
    prior affine in the depth (depth space) or in its inverse (disparity space) with noise, at least 0.01, exactly 0 at
    one pixel in nine.  prior: "noisy", "zero" (no valid pixel), "constant" (no correlation).
    -> float32 depth_acc [S,H,W], alphas [S,H,W], prior [H,W], depth [H,W]"""
    rng = np.random.default_rng(seed)
    depth = rng.uniform(2.0, 8.0, (H, W))
    covered = rng.uniform(size=(H, W)) >= 0.125
    if H * W <= 2:
        covered[:] = True
    al = rng.uniform(0.06, 1.0, (S, H, W)) * covered
    acc = al * depth * (1.0 + 0.05 * rng.standard_normal((S, H, W)))
    if space == "depth":
        pr = 0.37 * depth + 1.9 + 0.05 * rng.standard_normal((H, W))
    else:
        pr = 2.0 / depth + 0.1 + 0.01 * rng.standard_normal((H, W))
    pr = np.maximum(pr, 0.01)
    if H * W > 2:
        pr[rng.uniform(size=(H, W)) < 1.0 / 9.0] = 0.0
    if prior == "zero":
        pr[:] = 0.0
    elif prior == "constant":
        pr = np.where(pr > 0, 1.5, 0.0)
    else:
        assert prior == "noisy"
    return acc.astype(np.float32), al.astype(np.float32), pr.astype(np.float32), depth.astype(np.float32)


def make_batch(B, S, H, W, space, seed):
    """B frames; with B = 3 frame 1 has an all-zero prior and frame 2 a constant one.  -> depth_acc, alphas [B,S,H,W], prior
    [B,H,W], the kinds of the priors"""
    kinds = ["noisy", "zero", "constant"] if B == 3 else ["noisy"] * B
    frames = [make_frame(S, H, W, space, seed + 101 * b, kinds[b]) for b in range(B)]
    return (np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]), np.stack([f[2] for f in frames]), kinds)


def assert_input_conditions(depth_acc, alphas, prior, space, expect_degenerate):
    """what makes the product's and the reference's validity masks identical, and the frame well conditioned: alphas
    exactly 0 or >= 0.05, priors exactly 0 or >= 0.01, d exactly 0 where alpha is 0; a non-degenerate frame (with more
    than two pixels) has vx / (n sxx) >= 1e-3 and vy / (n syy) >= 1e-3"""
    S = alphas.shape[0]
    assert ((alphas == 0) | (alphas >= 0.05)).all() and ((prior == 0) | (prior >= 0.01)).all()
    r = reference(depth_acc, alphas, prior, "pearson", space, store=np.float32)
    d, a = depth_acc[0], alphas[0]
    for s in range(1, S):
        d, a = d + depth_acc[s], a + alphas[s]
    d, a = d / np.float32(S), a / np.float32(S)
    assert ((a == 0) | (a >= 0.05)).all() and (d[a == 0] == 0).all() and (d[a > 0] > 0).all()
    assert r["degenerate"] == expect_degenerate
    if not r["degenerate"]:
        n, sx, sy, sxx, syy = r["stats"][:5]
        assert (n * sxx - sx * sx) / (n * sxx) >= 1e-3 and (n * syy - sy * sy) / (n * syy) >= 1e-3
