"""TEST INFRASTRUCTURE (no tests here): the float64 yardstick of the colour fit behind the colour-corrected metrics
(3dgs-deblur_amd/colorcorrect.py, csrc/colorcorrect.hip), written with numpy from the statement of the algorithm in
csrc/colorcorrect_math.h, one image pair and one channel at a time.

reference(..., store=torch.float32) rounds the image to float32 after every iteration and decides the masks on those
float32 values, as the product does; store=None keeps float64 throughout (the masks then compare float64 values against
the same two thresholds).  The difference of the two is what float32 storage costs the reference itself: the tests'
bound is 4 x that + 1e-6.
"""
import numpy as np
import torch

EPS = 0.5 / 255
FEATURES = 10
MIN_COUNT = 10
PIVOT_TOL = 1e-10


def thresholds(eps=EPS):
    """(lo, hi) as float32 scalars: float(eps), float(1 - eps)"""
    return np.float32(eps), np.float32(1.0 - eps)


def features(x):
    """x [..., 3] -> float64 [..., 10]: rr, rg, rb, gg, gb, bb, r, g, b, 1"""
    x = np.asarray(x, np.float64)
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    return np.stack([r * r, r * g, r * b, g * g, g * b, b * b, r, g, b, np.ones_like(r)], axis=-1)


def identity_warp(c):
    w = np.zeros(FEATURES)
    w[6 + c] = 1.0
    return w


def solve_channel(G, h, c):
    """(w [10], fitted): the normal equations G w = h by Cholesky of the Jacobi-scaled matrix; the identity warp when
    fewer than MIN_COUNT rows took part (G[9,9] is their number), a diagonal entry is not positive, or a pivot of the
    scaled matrix is not above PIVOT_TOL"""
    G, h = np.asarray(G, np.float64), np.asarray(h, np.float64)
    n = FEATURES
    if not G[n - 1, n - 1] >= MIN_COUNT:
        return identity_warp(c), False
    diag = np.diag(G)
    if not np.all(diag > 0):
        return identity_warp(c), False
    d = 1.0 / np.sqrt(diag)
    S = G * d[:, None] * d[None, :]
    L = np.zeros((n, n))
    for j in range(n):
        s = S[j, j] - np.dot(L[j, :j], L[j, :j])
        if not s > PIVOT_TOL:
            return identity_warp(c), False
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, n):
            L[i, j] = (S[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    y = np.zeros(n)
    for i in range(n):
        y[i] = (h[i] * d[i] - np.dot(L[i, :i], y[:i])) / L[i, i]
    z = np.zeros(n)
    for i in range(n - 1, -1, -1):
        z[i] = (y[i] - np.dot(L[i + 1:, i], z[i + 1:])) / L[i, i]
    return z * d, True


def moments(x, mask, target):
    """masked normal equations of one channel: x [P,3], mask [P] bool, target [P] -> (G [10,10], h [10]) float64"""
    a = features(x)[mask]
    return a.T @ a, a.T @ np.asarray(target, np.float64)[mask]


def _one(img, ref, num_iters, eps, store):
    lo, hi = thresholds(eps)
    H, W, _ = img.shape
    img = np.asarray(img, np.float32).reshape(-1, 3)
    ref = np.asarray(ref, np.float32).reshape(-1, 3)

    def unclipped(z):
        return (z >= lo) & (z <= hi)
    fixed = unclipped(img) & unclipped(ref)
    x = img.copy() if store is not None else img.astype(np.float64)
    iterates = [x.reshape(H, W, 3).copy()]
    warps = np.zeros((num_iters, 3, FEATURES))
    for it in range(num_iters):
        mask = fixed & unclipped(x)
        for c in range(3):
            G, h = moments(x, mask[:, c], ref[:, c])
            warps[it, c], _ = solve_channel(G, h, c)
        x = np.clip(features(x) @ warps[it].T, 0.0, 1.0)
        if store is not None:
            x = x.astype(np.float32)
        iterates.append(x.reshape(H, W, 3).copy())
    return iterates, warps


def reference(img, ref, num_iters=5, eps=EPS, store=torch.float32, return_iterates=False):
    """img, ref: float32 tensors [H,W,3] or [B,H,W,3] -> (out float64 tensor of img's shape, warps float64
    [(B,) num_iters, 3, 10]); return_iterates: also the list of the num_iters + 1 images x_0 = img, ..., x_n = out"""
    if store not in (None, torch.float32):
        raise ValueError("store is torch.float32 or None")
    if img.dim() == 4:
        res = [reference(i, r, num_iters, eps, store, return_iterates) for i, r in zip(img, ref)]
        out = (torch.stack([r[0] for r in res]), torch.stack([r[1] for r in res]))
        return out + ([torch.stack(s) for s in zip(*[r[2] for r in res])],) if return_iterates else out
    iterates, warps = _one(img.detach().cpu().numpy(), ref.detach().cpu().numpy(), num_iters, eps, store)
    its = [torch.from_numpy(np.asarray(x, np.float64)) for x in iterates]
    out = (its[-1], torch.from_numpy(warps))
    return out + (its,) if return_iterates else out


def fragile(img, ref, num_iters=5, eps=EPS, tol=1e-6, iterates=None):
    """bool [(B,) H, W]: pixels with a value, in any channel of img, ref or any iterate of the float32-stored reference
    (computed here unless given), within tol of either threshold — where a rounding difference may flip a mask decision"""
    lo, hi = (float(v) for v in thresholds(eps))
    if iterates is None:
        iterates = reference(img, ref, num_iters, eps, torch.float32, return_iterates=True)[2]
    near = torch.zeros(img.shape[:-1], dtype=torch.bool)
    for t in [img.double().cpu(), ref.double().cpu()] + list(iterates):
        near |= (((t - lo).abs() <= tol) | ((t - hi).abs() <= tol)).any(-1)
    return near


SIZES = [(1, 1), (7, 5), (16, 12), (64, 48), (480, 270)]        # (W, H) of the accuracy tests, CPU and GPU
FRAGILE_FREE_UP_TO = 64 * 48                                     # up to here a case must have no fragile pixel at all
FRAGILE_CAP = 1e-4                                               # above: at most 0.01 % of the pixels
_CASES = {}


def seed_for(B, H, W):
    """seeds checked on the CPU: no fragile pixel at any size up to 64 x 48 or in the one-row cases of 255, 256 and 257
    pixels; 6 of 129 600 (B = 1) and 7 of 388 800 (B = 3) at 480 x 270"""
    return (5000 if H * W <= FRAGILE_FREE_UP_TO else 4000) + 100 * B + 3 * W + H


def case(B, H, W):
    """the shared, cached test case of this shape: inputs, both references and the fragile pixels; treat as read-only"""
    key = (B, H, W)
    if key not in _CASES:
        img, ref = random_case(B, H, W, seed_for(B, H, W))
        out32, w32, its = reference(img, ref, store=torch.float32, return_iterates=True)
        out64, w64 = reference(img, ref, store=None)
        _CASES[key] = dict(img=img, ref=ref, out32=out32, w32=w32, out64=out64, w64=w64,
                           fragile=int(fragile(img, ref, iterates=its).sum()))
    return _CASES[key]


def check_case(k, out, warps, what):
    """out [B,H,W,3], warps [B,5,3,10] of the code under test against reference(store=float32) of case k.  The bound is
    measured, not chosen: 4 x max |reference(store=float32) - reference(store=None)| on the same inputs (what float32
    storage between the iterations costs the reference itself; the 4 allows for another summation order) + 1e-6; for the
    warps the same rule relative to max |w|.  Prints every figure before it asserts."""
    B, H, W, _ = k["img"].shape
    n_px = B * H * W
    if H * W <= FRAGILE_FREE_UP_TO:
        assert k["fragile"] == 0, f"{what}: {k['fragile']} fragile pixels; pick another seed"
    else:
        assert k["fragile"] <= FRAGILE_CAP * n_px, f"{what}: {k['fragile']} of {n_px} pixels are fragile"
    e_ref = float((k["out32"] - k["out64"]).abs().max())
    e_out = float((out.detach().cpu().double() - k["out32"]).abs().max())
    bound = 4.0 * e_ref + 1e-6
    wmax = float(k["w32"].abs().max())
    e_wref = float((k["w32"] - k["w64"]).abs().max()) / wmax
    e_w = float((warps.detach().cpu().double() - k["w32"]).abs().max()) / wmax
    wbound = 4.0 * e_wref + 1e-6
    print(f"{what}: out err {e_out:.3e} (reference-only term {e_ref:.3e}, bound {bound:.3e}); warps rel err {e_w:.3e} "
          f"(reference-only term {e_wref:.3e}, bound {wbound:.3e}, max|w| {wmax:.3e}); fragile {k['fragile']}/{n_px}")
    assert e_out <= bound, (what, "out", e_out, bound)
    assert e_w <= wbound, (what, "warps", e_w, wbound)


def random_case(B, H, W, seed):
    """(img, ref) float32 [B,H,W,3]: ref = smooth colour fields plus noise with about 5 % of its pixels saturated to exactly
    0 or 1 (far from the thresholds); img = a mild affine + quadratic warp of ref plus noise, clipped, with another 2 % of
    its pixels saturated.  Every image of the batch has its own fields, warp and noise."""
    g = torch.Generator().manual_seed(seed)

    def rand(*s):
        return torch.rand(*s, generator=g, dtype=torch.float64)
    ys, xs = (torch.arange(H, dtype=torch.float64) + 0.5) / H, (torch.arange(W, dtype=torch.float64) + 0.5) / W
    yy, xx = torch.meshgrid(ys, xs, indexing="ij")
    imgs, refs = [], []
    for _ in range(B):
        f = 1.0 + 5.0 * rand(3, 2)
        ph = 6.28 * rand(3)
        ref = torch.stack([0.5 + 0.28 * torch.sin(f[c, 0] * xx + f[c, 1] * yy + ph[c]) for c in range(3)], dim=-1)
        ref = (ref + 0.08 * (rand(H, W, 3) - 0.5)).clamp(0.03, 0.97)
        sat = rand(H, W)
        ref[sat < 0.025] = 0.0
        ref[sat > 0.975] = 1.0
        A = torch.eye(3, dtype=torch.float64) * (0.8 + 0.3 * rand(1)) + 0.06 * (rand(3, 3) - 0.5)
        b = 0.06 * (rand(3) - 0.5)
        q = 0.1 * (rand(3) - 0.5)
        img = ref @ A.T + b + q * ref * ref.roll(1, -1) + 0.02 * (rand(H, W, 3) - 0.5)
        img = img.clamp(0.0, 1.0)
        sat = rand(H, W)
        img[sat < 0.01] = 0.0
        img[sat > 0.99] = 1.0
        imgs.append(img.float())
        refs.append(ref.float())
    return torch.stack(imgs), torch.stack(refs)
