"""TEST INFRASTRUCTURE: float64 reference of the per-frame blur statistics (csrc/blur_math.h, blurscore.py) and the
cases every implementation — the host build of the header, blur_stats_torch, the HIP kernels — is checked on.

reference(case)          every formula of the statistic in float64, from the float32 inputs.
reference_f32(case)      (a) the same formulas with every per-pair operation in numpy float32 and the sums in float64: what
                         ANY float32 implementation of this rounding chain can be expected to differ from the reference
                         by.  Its only use is to size the tolerance.
drop_fragile(case)       (b) the case without the points whose pixel lies within 1e-3 px of an image border, or whose depth
                         lies within 1e-4 of clip, in any frame: float32 and float64 may classify those differently.  Every
                         case loses at most 2 % of its points this way (asserted in cases()).
tolerance / check        per case and statistic tol = max(8 x |(a) - reference|, 4 x 2^-24 x |reference|); count is equal.
                         The 8 covers a different but equally long rounding chain (operation order, view transform), the
                         floor a few float32 ulps for max_blur and the final float32 rounding.

Measured (a) errors on these cases, relative to the reference, largest over all cases and frames (`python
tests/blur_reference.py` prints them per case; MEASURED below holds them and test_blur_host.py fails when it is out of
date): mean_blur 1.3e-7, rms_blur 1.3e-7, max_blur 2.3e-7, mean_skew 1.1e-6 — the last in the single-point case, whose
point lies near the middle row where v / H - 1/2 cancels; the means of the larger cases are at 1e-8 to 4e-8.  A case that
needed more than 1e-5 would be ill-conditioned (asserted in test_blur_host.py).  drop_fragile removes at most 2 of 3001
points.  The HIP kernels, the host build and blur_stats_torch form every per-pair value in the order (a) does, so their
errors are (a)'s plus the final float32 rounding.

exact_displacement(case) the convention pin's other side: the pixel distance between a point's projections at the two ends
                         of the exposure, through the exact SE(3) screw viewmat(t) = Exp(-t xi) viewmat, per-frame mean
                         over the pairs visible at mid-exposure.
"""
import numpy as np

CLIP = 0.01
W, H, FOCAL = 64, 48, 60.0
E0, T0 = 0.02, 0.03
CHUNK, FRAME_GROUP = 1024, 32            # csrc/blur_math.h kChunk, kFrameGroup (test_blur_host.py pins them)
STATS = ("mean_blur", "rms_blur", "max_blur", "mean_skew")

# largest relative |(a) - reference| over all cases, per statistic (python tests/blur_reference.py prints them)
MEASURED = {"mean_blur": 1.4e-07, "rms_blur": 1.4e-07, "max_blur": 2.4e-07, "mean_skew": 1.2e-06}


# --------------------------------------------------------------------------- #
# cases
# --------------------------------------------------------------------------- #
def look_at(eye, target, up=(0.0, -1.0, 0.0)):
    """world-to-camera [4,4] float64 in OpenCV axes (x right, y down, z forward)"""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(-up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    V = np.eye(4)
    V[:3, :3] = R
    V[:3, 3] = -R @ eye
    return V


def circle_cameras(F, rng, radius=4.0):
    th = 2 * np.pi * (np.arange(F) + 0.25) / F
    eyes = np.stack([radius * np.cos(th), 0.6 * np.sin(3 * th), radius * np.sin(th)], 1)
    return np.stack([look_at(e, rng.uniform(-0.2, 0.2, 3)) for e in eyes])


def make_case(name, N=3001, F=7, seed=0):
    rng = np.random.default_rng(1000 + seed)
    c = {"name": name, "W": W, "H": H, "clip": CLIP}
    c["points"] = rng.uniform(-1.5, 1.5, (3001, 3))[:N]
    c["viewmats"] = circle_cameras(F, rng)
    c["lin"] = rng.uniform(-0.5, 0.5, (F, 3))
    c["ang"] = rng.uniform(-0.6, 0.6, (F, 3))
    c["intrins"] = np.tile(np.array([FOCAL, FOCAL, W / 2.0, H / 2.0]), (F, 1))
    c["times"] = np.tile(np.array([E0, T0]), (F, 1))
    return c


def _f32(c):
    return {k: (np.ascontiguousarray(v, dtype=np.float32) if isinstance(v, np.ndarray) else v) for k, v in c.items()}


_CASES = None


def cases():
    """[case]: name, points [N,3], viewmats [F,4,4], lin / ang [F,3], intrins [F,4], times [F,2] (float32), W, H, clip;
    built once, fragile points dropped, never modified"""
    global _CASES
    if _CASES is not None:
        return _CASES
    out = []
    for i, N in enumerate((1, 63, 257, CHUNK - 1, CHUNK, CHUNK + 1, 3001)):
        out.append(make_case(f"N{N}", N=N, seed=i))
    for i, F in enumerate((1, FRAME_GROUP - 1, FRAME_GROUP, FRAME_GROUP + 1)):
        out.append(make_case(f"F{F}", N=CHUNK + 1, F=F, seed=10 + i))
    c = make_case("looking_away", seed=20)                   # frame 3 turns its back on the cloud: count 0, zeros out
    c["viewmats"][3, :3] = np.diag([-1.0, 1.0, -1.0]) @ c["viewmats"][3, :3]
    out.append(c)
    c = make_case("behind_camera_0", seed=21)                # a small cloud wholly behind camera 0; others may see it
    eye0 = -c["viewmats"][0, :3, :3].T @ c["viewmats"][0, :3, 3]
    c["points"] = c["points"] * 0.2 + 1.5 * eye0
    out.append(c)
    c = make_case("zeros", seed=22)                          # exact zeros: E = 0, T = 0, no twist, both times 0
    c["times"][0, 0] = 0.0                                   # frame 0 is T-only
    c["times"][1, 1] = 0.0                                   # frame 1 is E-only
    c["lin"][2] = 0.0
    c["ang"][2] = 0.0
    c["times"][3] = 0.0
    out.append(c)
    c = make_case("intrinsics", seed=23)                     # every frame its own fx fy cx cy
    rng = np.random.default_rng(5)
    c["intrins"] = np.stack([rng.uniform(45, 90, 7), rng.uniform(45, 90, 7), rng.uniform(25, 40, 7),
                             rng.uniform(18, 30, 7)], 1)
    c["times"] = np.stack([rng.uniform(0.005, 0.03, 7), rng.uniform(0.01, 0.04, 7)], 1)
    out.append(c)
    done = []
    for c in out:
        c = _f32(c)
        kept = drop_fragile(c)
        n = c["points"].shape[0]
        assert n - kept["points"].shape[0] <= 0.02 * n, (c["name"], n, kept["points"].shape[0])
        done.append(kept)
    _CASES = done
    return done


# --------------------------------------------------------------------------- #
# the statistic
# --------------------------------------------------------------------------- #
def _pairs(c, dt):
    """per-pair values [F,N] with every operation in dtype dt, in the order of csrc/blur_math.h"""
    t = lambda a: np.asarray(a, dtype=dt)
    p = t(c["points"])
    px, py, pz = p[None, :, 0], p[None, :, 1], p[None, :, 2]
    V = t(c["viewmats"]).reshape(-1, 16)
    v = [V[:, k, None] for k in range(12)]
    lin, ang = ([t(c[k])[:, a, None] for a in range(3)] for k in ("lin", "ang"))
    fx, fy, cx, cy = (t(c["intrins"])[:, a, None] for a in range(4))
    E, T = t(c["times"])[:, 0, None], t(c["times"])[:, 1, None]
    Wd, Hd, clip, half, one = dt(c["W"]), dt(c["H"]), dt(np.float32(c["clip"])), dt(0.5), dt(1.0)
    with np.errstate(all="ignore"):
        pcx = ((v[0] * px + v[1] * py) + v[2] * pz) + v[3]
        pcy = ((v[4] * px + v[5] * py) + v[6] * pz) + v[7]
        pcz = ((v[8] * px + v[9] * py) + v[10] * pz) + v[11]
        rz = one / pcz
        u = (fx * pcx) * rz + cx
        vv = (fy * pcy) * rz + cy
        ux = -(ang[1] * pcz - ang[2] * pcy) - lin[0]
        uy = -(ang[2] * pcx - ang[0] * pcz) - lin[1]
        uz = -(ang[0] * pcy - ang[1] * pcx) - lin[2]
        rz2 = rz * rz
        pvx = (fx * rz) * ux - ((fx * pcx) * rz2) * uz
        pvy = (fy * rz) * uy - ((fy * pcy) * rz2) * uz
        mag = np.sqrt(pvx * pvx + pvy * pvy)
        blur = E * mag
        skew = (T * mag) * np.abs(vv / Hd - half)
        vis = (pcz > clip) & (u >= 0) & (u < Wd) & (vv >= 0) & (vv < Hd)
    for a in (pcx, rz, u, blur, skew):
        assert a.dtype == dt, a.dtype
    return dict(pcz=pcz, u=u, v=vv, blur=blur, skew=skew, vis=vis)


def _reduce(q):
    vis = q["vis"]
    n = vis.sum(1)
    nd = np.maximum(n, 1).astype(np.float64)
    b = np.where(vis, q["blur"].astype(np.float64), 0.0)
    s = np.where(vis, q["skew"].astype(np.float64), 0.0)
    some = n > 0
    return {"count": n.astype(np.int32), "mean_blur": np.where(some, b.sum(1) / nd, 0.0),
            "rms_blur": np.where(some, np.sqrt((b * b).sum(1) / nd), 0.0), "max_blur": b.max(1, initial=0.0),
            "mean_skew": np.where(some, s.sum(1) / nd, 0.0)}


_REF = {}


def reference(c):
    """{count [F] int32, mean_blur, rms_blur, max_blur, mean_skew [F] float64}; computed once per case"""
    hit = _REF.get(c["name"])
    if hit is None:
        hit = _REF[c["name"]] = (_reduce(_pairs(c, np.float64)), _reduce(_pairs(c, np.float32)))
    return hit[0]


def reference_f32(c):
    reference(c)
    return _REF[c["name"]][1]


def drop_fragile(c):
    q = _pairs(c, np.float64)
    near = lambda a, b: np.abs(a - b) < 1e-3
    fragile = (near(q["u"], 0) | near(q["u"], c["W"]) | near(q["v"], 0) | near(q["v"], c["H"])
               | (np.abs(q["pcz"] - np.float64(np.float32(c["clip"]))) < 1e-4)).any(0)
    out = dict(c)
    out["points"] = np.ascontiguousarray(c["points"][~fragile])
    return out


def tolerance(c):
    ref, a = reference(c), reference_f32(c)
    assert np.array_equal(ref["count"], a["count"]), c["name"]         # what drop_fragile is for
    return {k: np.maximum(8.0 * np.abs(a[k] - ref[k]), 4.0 * 2.0 ** -24 * np.abs(ref[k])) for k in STATS}


def check(c, got, what=""):
    """got: {count, mean_blur, rms_blur, max_blur, mean_skew} arrays [F] of an implementation under test"""
    ref, tol = reference(c), tolerance(c)
    cnt = np.asarray(got["count"])
    assert np.array_equal(cnt.astype(np.int64), ref["count"].astype(np.int64)), (what, c["name"], cnt, ref["count"])
    for k in STATS:
        g = np.asarray(got[k], dtype=np.float64)
        err = np.abs(g - ref[k])
        print(f"{what} {c['name']} {k}: max err {err.max():.3e} (tol there {tol[k][err.argmax()]:.3e})")
        assert (err <= tol[k]).all(), (what, c["name"], k, err.max(), tol[k][err.argmax()], g, ref[k])


def measured_errors():
    """{statistic: the largest |(a) - reference| / |reference| over all cases and frames}"""
    out = {k: 0.0 for k in STATS}
    for c in cases():
        ref, a = reference(c), reference_f32(c)
        for k in STATS:
            nz = ref[k] != 0
            if nz.any():
                out[k] = max(out[k], float((np.abs(a[k] - ref[k])[nz] / np.abs(ref[k][nz])).max()))
    return out


# --------------------------------------------------------------------------- #
# the convention pin: first order against the exact screw
# --------------------------------------------------------------------------- #
def _se3_exp(v, w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)
    if th < 1e-6:
        A, B, C = 1 - th * th / 6, 0.5 - th * th / 24, 1 / 6 - th * th / 120
    else:
        A, B, C = np.sin(th) / th, (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    E = np.eye(4)
    E[:3, :3] = np.eye(3) + A * K + B * K @ K
    E[:3, 3] = (np.eye(3) + B * K + C * K @ K) @ v
    return E


def subpose(V, lin, ang, t):
    """viewmat(t) = Exp(-t xi) viewmat, float64 (csrc/gs_math.h subpose_viewmat)"""
    return _se3_exp(-t * np.asarray(lin, np.float64), -t * np.asarray(ang, np.float64)) @ np.asarray(V, np.float64)


def exact_displacement(c, margin=0.0):
    """(mean over the pairs visible at mid-exposure — at least `margin` px inside the image — of the pixel distance between
    the projections at t = -E/2 and t = +E/2 [F], the first-order mean_blur over the same pairs [F], that selection
    [F,N]), float64"""
    q = _pairs(c, np.float64)
    sel = q["vis"] & (q["u"] >= margin) & (q["u"] < c["W"] - margin) & (q["v"] >= margin) & (q["v"] < c["H"] - margin)
    p = np.concatenate([c["points"].astype(np.float64), np.ones((c["points"].shape[0], 1))], 1)
    F = c["viewmats"].shape[0]
    exact, first = np.zeros(F), np.zeros(F)
    for f in range(F):
        fx, fy, cx, cy = c["intrins"][f].astype(np.float64)
        E = float(c["times"][f, 0])
        ends = []
        for t in (-0.5 * E, 0.5 * E):
            pc = p[sel[f]] @ subpose(c["viewmats"][f], c["lin"][f], c["ang"][f], t).T
            ends.append(np.stack([fx * pc[:, 0] / pc[:, 2] + cx, fy * pc[:, 1] / pc[:, 2] + cy], 1))
        exact[f] = np.linalg.norm(ends[1] - ends[0], axis=1).mean()
        first[f] = q["blur"][f][sel[f]].mean()
    return exact, first, sel


def pin_case():
    """the base scene with its twists scaled down until the first-order streak and the exact displacement agree to 1 % in
    every frame (asserted): -> (case, scale)"""
    base = _f32(make_case("pin", seed=30))
    scale = 1.0
    while True:
        c = dict(base, lin=base["lin"] * np.float32(scale), ang=base["ang"] * np.float32(scale))
        exact, first, sel = exact_displacement(c, margin=2.0)
        assert sel.sum(1).min() >= 100
        if (np.abs(exact - first) < 0.01 * first).all():
            return c, scale
        scale *= 0.5
        assert scale > 1e-3, "the first-order model never meets the exact screw: a convention is wrong"


if __name__ == "__main__":
    for c in cases():
        ref, a = reference(c), reference_f32(c)
        rel = {k: float(np.max(np.abs(a[k] - ref[k]) / np.maximum(np.abs(ref[k]), 1e-300))) for k in STATS}
        print(c["name"], c["points"].shape[0], "points", c["viewmats"].shape[0], "frames, count", ref["count"].min(), "..",
              ref["count"].max(), {k: f"{v:.1e}" for k, v in rel.items()})
    print("largest:", {k: f"{v:.2e}" for k, v in measured_errors().items()})
    c, s = pin_case()
    exact, first, _ = exact_displacement(c, 2.0)
    print("pin scale", s, "gap", np.abs(exact - first) / first)
