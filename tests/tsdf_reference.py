"""Float64 reference of TSDF fusion and marching-tetrahedra extraction (tsdf.py), written from the stated rules, not from
the kernels: plain loops, nothing shared with csrc/tsdf_math.h or tsdf.py.  Also the scenes of the tests and the mesh checks.

INTEGRATE  integrate(...) loops over voxels and frames.  It also marks the FRAGILE voxels: nearest-pixel and cut-off
decisions are discontinuous, so a voxel is left out of a comparison when, for any frame, a pixel coordinate is within
2e-4 px of an integer, |sdf + trunc| < 1e-5 D, or D is within 1e-6 relative of a depth bound.
integrate_frames(...) is the same rule one frame at a time over whole arrays (for the 48^3 end-to-end bound).

EXTRACT    extract(...) loops over the cells whose corners are not all on one side.  The orientation of a triangle is found
geometrically (its normal against the direction from the inside corners to the outside ones, at edge midpoints: the
parity does not depend on the values), not from a table."""
import functools
import itertools
import math

import numpy as np

FRAGILE_PIXEL = 2e-4
FRAGILE_SDF = 1e-5
FRAGILE_BOUND = 1e-6
FRAGILE_CAP = 0.03

AXIS_ORDERS = list(itertools.permutations(range(3)))          # xyz, xzy, yxz, yzx, zxy, zyx
EDGE_TYPES = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]


# ---- scenes -------------------------------------------------------------------------------------------------------------
def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """world-to-camera 4x4, OpenCV axes (x right, y down, z forward)"""
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    fwd = target - eye
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    m = np.eye(4)
    m[:3, :3] = np.stack([right, down, fwd])
    m[:3, 3] = -m[:3, :3] @ eye
    return m


def ring_cameras(B, radius=2.5, target=(0.0, 0.0, 0.0), height=0.35, phase=0.1):
    return np.stack([look_at((target[0] + radius * math.cos(phase + 2 * math.pi * b / B),
                              target[1] + radius * math.sin(phase + 2 * math.pi * b / B), target[2] + height), target)
                     for b in range(B)]).astype(np.float32)


def smooth_images(B, H, W, seed):
    """depth [B,H,W] around the ring radius, colour [B,H,W,3] in [0, 1], float32, smooth in the pixel"""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing="ij")
    depth = np.empty((B, H, W), np.float32)
    color = np.empty((B, H, W, 3), np.float32)
    for b in range(B):
        a = rng.uniform(-1, 1, 6)
        depth[b] = 2.5 + 0.25 * np.sin(3 * xx + 6 * a[0]) * np.cos(2 * yy + 6 * a[1]) + 0.2 * a[2] * xx + 0.2 * a[3] * yy
        for c in range(3):
            color[b, :, :, c] = 0.5 + 0.5 * np.sin(4 * xx * a[4] + 5 * yy * a[5] + c + b)
    return depth, color


SMALL = dict(origin=(-1.0, -0.5, -0.25), voxel_size=0.0625, dims=(33, 17, 9))     # centred on the origin
SMALL_IMAGE = (32, 48)                                                             # H, W
SMALL_INTRIN = (40.0, 40.0, 24.0, 16.0)
SMALL_TRUNC = 0.25


def small_scene(B, seed=0):
    """B ring cameras around the 33 x 17 x 9 volume -> depth, color, viewmats, intrins (float32)"""
    H, W = SMALL_IMAGE
    depth, color = smooth_images(B, H, W, seed)
    return depth, color, ring_cameras(B), np.tile(np.float32(SMALL_INTRIN), (B, 1))


@functools.lru_cache(maxsize=None)
def cached_small(frames_per_launch):
    """the ring scene of frames_per_launch + 1 cameras, shared by the host and the GPU tests; a case of B frames takes the
    first B -> (scene, {B: integrate's result after B frames} for B in small_counts(frames_per_launch))"""
    scene = small_scene(frames_per_launch + 1)
    depth, color, views, intr = scene
    return scene, integrate(SMALL["origin"], SMALL["voxel_size"], SMALL["dims"], depth, views, intr, SMALL_TRUNC, color=color,
                            snapshots=small_counts(frames_per_launch))


def small_counts(frames_per_launch):
    return (1, 3, frames_per_launch - 1, frames_per_launch, frames_per_launch + 1)


@functools.lru_cache(maxsize=None)
def cached_hard():
    depth, color, weights, views, intr, depth_max = hard_scene()
    return integrate(SMALL["origin"], SMALL["voxel_size"], SMALL["dims"], depth, views, intr, SMALL_TRUNC, color=color,
                     weights=weights, depth_min=0.5, depth_max=depth_max)


def hard_scene():
    """the further case: a camera inside the volume (voxels behind it), a camera that sees half of the volume, and
    pixels that are NaN, zero, beyond depth_max and of weight 0 -> depth, color, weights, viewmats, intrins, depth_max"""
    H, W = SMALL_IMAGE
    depth, color = smooth_images(4, H, W, 7)
    views = ring_cameras(4)
    views[1] = look_at((0.31, 0.07, 0.02), (-2.0, 0.4, 0.1)).astype(np.float32)          # inside the volume
    views[2] = look_at((2.5, 0.3, 0.4), (2.0, 2.5, 0.0)).astype(np.float32)              # sees about half of it
    depth[1] = depth[1] - 1.9                                                             # a surface inside the volume
    weights = np.ones((4, H, W), np.float32)
    depth[0, 13:16, 12:20] = np.nan
    depth[0, 16:18, 28:36] = np.inf
    depth[3, 14:18, 14:22] = 0.0
    depth[2, 0:16, :] = 2.9                                                               # beyond depth_max
    weights[3, 12:20, 26:34] = 0.0
    weights[0, :, 24:] = 0.5
    return depth, color, weights, views, np.tile(np.float32(SMALL_INTRIN), (4, 1)), 2.8


# ---- integration --------------------------------------------------------------------------------------------------------
def new_volume(dims, color=True):
    nx, ny, nz = dims
    return (np.ones((nz, ny, nx)), np.zeros((nz, ny, nx)), np.zeros((nz, ny, nx, 3)) if color else None)


def integrate(origin, voxel_size, dims, depth, viewmats, intrins, trunc, color=None, weights=None, depth_min=0.0,
              depth_max=math.inf, max_weight=64.0, state=None, snapshots=None):
    """-> (tsdf, weight, color or None, fragile [nz,ny,nx] bool), float64; snapshots (frame counts): instead a dict
    {count: that tuple after the first `count` frames}"""
    nx, ny, nz = dims
    B, H, W = depth.shape
    tsdf, wgt, col = new_volume(dims, color is not None) if state is None else [None if a is None else a.copy() for a in state]
    fragile = np.zeros((nz, ny, nx), bool)
    snaps = {n: (tsdf.copy(), wgt.copy(), None if col is None else col.copy(), fragile.copy()) for n in (snapshots or ())}
    depth = depth.astype(np.float64)
    views = viewmats.astype(np.float64)
    K = intrins.astype(np.float64)
    o = [float(np.float32(a)) for a in origin]
    vs = float(np.float32(voxel_size))
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                x = np.array([o[0] + vs * i, o[1] + vs * j, o[2] + vs * k])
                f, Wt = tsdf[k, j, i], wgt[k, j, i]
                c = None if col is None else col[k, j, i].copy()
                for b in range(B + 1):
                    if b in snaps:
                        snaps[b][0][k, j, i], snaps[b][1][k, j, i], snaps[b][3][k, j, i] = f, Wt, fragile[k, j, i]
                        if c is not None:
                            snaps[b][2][k, j, i] = c
                    if b == B:
                        break
                    p = views[b, :3, :3] @ x + views[b, :3, 3]
                    z = p[2]
                    if z <= 0:
                        continue
                    u = K[b, 0] * p[0] / z + K[b, 2]
                    v = K[b, 1] * p[1] / z + K[b, 3]
                    if abs(u - round(u)) < FRAGILE_PIXEL or abs(v - round(v)) < FRAGILE_PIXEL:
                        fragile[k, j, i] = True
                    px, py = math.floor(u), math.floor(v)
                    if px < 0 or py < 0 or px >= W or py >= H:
                        continue
                    D = depth[b, py, px]
                    w = 1.0 if weights is None else float(weights[b, py, px])
                    if not math.isfinite(D):
                        continue
                    for bound in (depth_min, depth_max):
                        if math.isfinite(bound) and abs(D - bound) < FRAGILE_BOUND * abs(bound):
                            fragile[k, j, i] = True
                    if not (depth_min < D <= depth_max and w > 0):
                        continue
                    sdf = D - z
                    if abs(sdf + trunc) < FRAGILE_SDF * D:
                        fragile[k, j, i] = True
                    if sdf < -trunc:
                        continue
                    val = min(1.0, sdf / trunc)
                    Wn = Wt + w
                    f = (f * Wt + val * w) / Wn
                    if c is not None:
                        c = (c * Wt + color[b, py, px].astype(np.float64) * w) / Wn
                    Wt = min(Wn, max_weight)
                tsdf[k, j, i], wgt[k, j, i] = f, Wt
                if c is not None:
                    col[k, j, i] = c
    if snapshots is not None:
        return snaps
    return tsdf, wgt, col, fragile


def integrate_frames(origin, voxel_size, dims, depth, viewmats, intrins, trunc, depth_min=0.0, depth_max=math.inf,
                     max_weight=64.0):
    """the same rule without colour or weights, one frame at a time over the whole volume -> (tsdf, weight)"""
    nx, ny, nz = dims
    B, H, W = depth.shape
    o = [float(np.float32(a)) for a in origin]
    vs = float(np.float32(voxel_size))
    zz, yy, xx = np.meshgrid(o[2] + vs * np.arange(nz), o[1] + vs * np.arange(ny), o[0] + vs * np.arange(nx), indexing="ij")
    tsdf, wgt = np.ones((nz, ny, nx)), np.zeros((nz, ny, nx))
    for b in range(B):
        m, K = viewmats[b].astype(np.float64), intrins[b].astype(np.float64)
        p = [m[r, 0] * xx + m[r, 1] * yy + m[r, 2] * zz + m[r, 3] for r in range(3)]
        ok = p[2] > 0
        z = np.where(ok, p[2], 1.0)
        px, py = np.floor(K[0] * p[0] / z + K[2]), np.floor(K[1] * p[1] / z + K[3])
        ok &= (px >= 0) & (py >= 0) & (px < W) & (py < H)
        D = depth[b].astype(np.float64)[np.where(ok, py, 0).astype(int), np.where(ok, px, 0).astype(int)]
        with np.errstate(invalid="ignore"):
            ok &= np.isfinite(D) & (D > depth_min) & (D <= depth_max)
            sdf = D - z
            ok &= ~(sdf < -trunc)
            val = np.minimum(1.0, sdf / trunc)
        Wn = np.where(ok, wgt + 1.0, 1.0)
        tsdf = np.where(ok, (tsdf * wgt + np.where(ok, val, 0.0)) / Wn, tsdf)
        wgt = np.where(ok, np.minimum(Wn, max_weight), wgt)
    return tsdf, wgt


def check_volume(got, ref, what, atol=1e-5):
    """got: (tsdf, weight, color or None) float32 arrays; ref: integrate's result.  tsdf and colour within atol outside
    the fragile voxels, weight exact there, untouched voxels exactly (1, 0, 0); at most 3 % fragile."""
    tsdf, wgt, col, fragile = ref
    share = float(fragile.mean())
    print(f"{what}: fragile {100 * share:.2f} % of {fragile.size} voxels, touched {int((wgt > 0).sum())}")
    assert share <= FRAGILE_CAP, (what, share)
    keep = ~fragile
    assert (wgt > 0).sum() > 0.2 * wgt.size, what                       # the scene does reach the volume
    assert np.array_equal(np.asarray(got[1], np.float64)[keep], wgt[keep]), what
    err = np.abs(np.asarray(got[0], np.float64) - tsdf)[keep].max()
    print(f"{what}: max |tsdf error| {err:.3g}")
    assert err <= atol, (what, err)
    untouched = keep & (wgt == 0)
    assert (np.asarray(got[0])[untouched] == 1.0).all() and (np.asarray(got[1])[untouched] == 0.0).all(), what
    if col is not None:
        cerr = np.abs(np.asarray(got[2], np.float64) - col)[keep].max()
        print(f"{what}: max |colour error| {cerr:.3g}")
        assert cerr <= atol, (what, cerr)
        assert (np.asarray(got[2])[untouched] == 0.0).all(), what


# ---- extraction ---------------------------------------------------------------------------------------------------------
def extract(origin, voxel_size, tsdf, weight, color=None, level=0.0, min_weight=0.0):
    """tsdf, weight [nz,ny,nx] (float32 or float64), color [nz,ny,nx,3] or None -> (verts float64 [V,3], faces int64 [F,3],
    colors float64 [V,3] or None, cells [F] the linear index of every face's cell)"""
    f = np.asarray(tsdf, np.float64)
    w = np.asarray(weight, np.float64)
    nz, ny, nx = f.shape
    inside = f < level
    lo = np.ones((nz - 1, ny - 1, nx - 1), bool)
    hi = np.zeros((nz - 1, ny - 1, nx - 1), bool)
    for dz, dy, dx in itertools.product((0, 1), repeat=3):
        part = inside[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
        lo &= part
        hi |= part
    tris, cells = [], []
    for k, j, i in np.argwhere(hi & ~lo).tolist():                       # crossed cells, in linear order
        base = (i, j, k)
        if not all(w[k + dz, j + dy, i + dx] > min_weight for dz, dy, dx in itertools.product((0, 1), repeat=3)):
            continue
        for order in AXIS_ORDERS:
            path = [np.array(base)]
            for axis in order:
                step = np.zeros(3, int)
                step[axis] = 1
                path.append(path[-1] + step)
            ins = [n for n in range(4) if inside[path[n][2], path[n][1], path[n][0]]]
            out = [n for n in range(4) if n not in ins]
            if len(ins) in (0, 4):
                continue
            if len(ins) == 1:
                found = [[(ins[0], q) for q in out]]
            elif len(ins) == 3:
                found = [[(out[0], q) for q in ins]]
            else:
                (a, b), (c, d) = ins, out
                found = [[(a, c), (a, d), (b, d)], [(a, c), (b, d), (b, c)]]
            towards_free = np.mean([path[n] for n in out], axis=0) - np.mean([path[n] for n in ins], axis=0)
            for tri in found:
                mid = [(path[p] + path[q]) / 2.0 for p, q in tri]
                if np.dot(np.cross(mid[1] - mid[0], mid[2] - mid[0]), towards_free) < 0:
                    tri = [tri[0], tri[2], tri[1]]
                keys = []
                for p, q in tri:
                    p, q = min(p, q), max(p, q)
                    oi, oj, ok_ = path[p]
                    keys.append(((int(ok_) * ny + int(oj)) * nx + int(oi), EDGE_TYPES.index(tuple(path[q] - path[p]))))
                tris.append(keys)
                cells.append((k * ny + j) * nx + i)
    order = sorted({e for t in tris for e in t})
    index = {e: n for n, e in enumerate(order)}
    faces = np.array([[index[e] for e in t] for t in tris], np.int64).reshape(-1, 3)
    verts = np.zeros((len(order), 3))
    cols = None if color is None else np.zeros((len(order), 3))
    o = np.array([float(np.float32(a)) for a in origin])
    vs = float(np.float32(voxel_size))
    for n, (owner, etype) in enumerate(order):
        a = np.array([owner % nx, (owner // nx) % ny, owner // (nx * ny)])
        b = a + np.array(EDGE_TYPES[etype])
        fa, fb = f[a[2], a[1], a[0]], f[b[2], b[1], b[0]]
        t = (level - fa) / (fb - fa)
        pa, pb = o + vs * a, o + vs * b
        verts[n] = pa + t * (pb - pa)
        if cols is not None:
            ca, cb = (np.asarray(color[q[2], q[1], q[0]], np.float64) for q in (a, b))
            cols[n] = ca + t * (cb - ca)
    return verts, faces, cols, np.array(cells, np.int64)


def check_mesh(got, ref, what, rtol=1e-6):
    """got: (verts, faces, colors or None) arrays; ref: extract's result.  verts within rtol, faces exactly"""
    verts, faces, cols, _ = ref
    gv, gf = np.asarray(got[0], np.float64), np.asarray(got[1])
    assert gv.shape == verts.shape and gf.shape == faces.shape, (what, gv.shape, verts.shape, gf.shape, faces.shape)
    assert np.array_equal(gf.astype(np.int64), faces), what
    if len(verts):
        rel = np.abs(gv - verts) / np.abs(verts)
        print(f"{what}: V {len(verts)}, F {len(faces)}, max relative vertex error {rel.max():.3g}")
        assert np.allclose(gv, verts, rtol=rtol, atol=0.0), (what, rel.max())
    if cols is not None:
        assert np.allclose(np.asarray(got[2], np.float64), cols, rtol=0.0, atol=1e-6), what


def edge_uses(faces):
    """{(a, b) directed: count}"""
    uses = {}
    for a, b, c in np.asarray(faces).tolist():
        for e in ((a, b), (b, c), (c, a)):
            uses[e] = uses.get(e, 0) + 1
    return uses


def is_closed(faces):
    """every undirected edge in exactly two faces, once in each direction"""
    uses = edge_uses(faces)
    return len(uses) > 0 and all(n == 1 and uses.get((b, a), 0) == 1 for (a, b), n in uses.items())


def boundary_edges(faces):
    """(edges in exactly one face, edges in more than two faces or used twice in one direction)"""
    uses = edge_uses(faces)
    single = sum(1 for (a, b), n in uses.items() if n == 1 and (b, a) not in uses)
    bad = sum(1 for (a, b), n in uses.items() if n > 1 or n + uses.get((b, a), 0) > 2)
    return single, bad


def euler(verts, faces):
    edges = {(min(a, b), max(a, b)) for (a, b) in edge_uses(faces)}
    return len(verts) - len(edges) + len(faces)


def face_areas(verts, faces):
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces)
    return 0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


MESH_ORIGIN = (1.0, 2.0, 3.0)          # every coordinate well away from 0: rtol alone then bounds the vertex error


def grid_points(n, origin=MESH_ORIGIN, voxel_size=1.0):
    nx, ny, nz = (n, n, n) if isinstance(n, int) else n
    zz, yy, xx = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64),
                             np.arange(nx, dtype=np.float64), indexing="ij")
    return origin[0] + voxel_size * xx, origin[1] + voxel_size * yy, origin[2] + voxel_size * zz


SPHERE_C, SPHERE_R = (12.63, 13.41, 14.27), 8.0
TORUS_C, TORUS_R, TORUS_r = (12.63, 13.41, 14.27), 7.0, 2.6


def sphere_field(n=24, c=SPHERE_C, r=SPHERE_R, scale=4.0, voxel_size=1.0):
    """float32 tsdf of a sphere, truncated like a fused one: clip(distance / scale, -1, 1)"""
    x, y, z = grid_points(n, voxel_size=voxel_size)
    d = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r
    return np.clip(d / scale, -1.0, 1.0).astype(np.float32)


def torus_field(n=24, c=TORUS_C, R=TORUS_R, r=TORUS_r, scale=4.0):
    x, y, z = grid_points(n)
    q = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2) - R
    return np.clip((np.sqrt(q * q + (z - c[2]) ** 2) - r) / scale, -1.0, 1.0).astype(np.float32)


def field_colors(shape):
    nz, ny, nx = shape
    x, y, z = grid_points((nx, ny, nz))
    return np.stack([0.5 + 0.5 * np.sin(0.3 * x), 0.5 + 0.5 * np.cos(0.2 * y), 0.5 + 0.5 * np.sin(0.25 * z + 1.0)],
                    axis=-1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def cached_extract(name, dims=None):
    """the shared references of the host and the GPU tests -> (tsdf float32, weight float32, color float32, extract(...))"""
    if name == "sphere":
        f = sphere_field()
    elif name == "torus":
        f = torus_field()
    elif name == "blocks":                 # a thin tilted tube along z: it crosses every slab of a volume of the given dims
        x, y, z = grid_points(dims)
        r = min(2.6, 0.3 * min(dims[0], dims[1]))
        ax, ay = 1.0 + 0.43 * dims[0] + 0.011 * (z - 3.0), 2.0 + 0.52 * dims[1] - 0.007 * (z - 3.0)
        f = np.clip((np.sqrt((x - ax) ** 2 + (y - ay) ** 2) - r) / 4.0, -1.0, 1.0).astype(np.float32)
    else:
        raise KeyError(name)
    w = np.ones_like(f)
    col = field_colors(f.shape)
    return f, w, col, extract(MESH_ORIGIN, 1.0, f, w, col)


# ---- end to end: ray-cast sphere ------------------------------------------------------------------------------------------
def raycast_sphere_depth(viewmats, intrins, H, W, center, radius, far=8.0):
    """z-depth [B,H,W] float32 of a sphere seen through the pixel centres, a backdrop at `far` where the ray misses"""
    B = len(viewmats)
    out = np.full((B, H, W), far, np.float32)
    for b in range(B):
        m = viewmats[b].astype(np.float64)
        fx, fy, cx, cy = intrins[b].astype(np.float64)
        cc = m[:3, :3] @ np.asarray(center, np.float64) + m[:3, 3]              # the centre in camera space
        v, u = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
        d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], axis=-1)     # z-depth = the ray parameter
        a = (d * d).sum(-1)
        bq = d @ cc
        disc = bq * bq - a * (cc @ cc - radius * radius)
        hit = disc > 0
        s = (bq - np.sqrt(np.where(hit, disc, 0.0))) / a
        out[b] = np.where(hit & (s > 0), s, far).astype(np.float32)
    return out


def e2e_scene(n, B=12):
    """a sphere in an n^3 volume of side 2 seen by B ring cameras -> (origin, voxel_size, dims, depth, viewmats,
    intrins, trunc, center, radius)"""
    vs = 2.0 / (n - 1)
    origin = (-1.0, -1.0, -1.0)
    center, radius = (0.03, -0.02, 0.04), 0.6
    H, W = 96, 96
    views = np.concatenate([ring_cameras(B - 4, radius=2.5, target=center, height=0.6),
                            ring_cameras(2, radius=1.0, target=center, height=2.3, phase=0.4),
                            ring_cameras(2, radius=1.0, target=center, height=-2.3, phase=1.3)])
    intr = np.tile(np.float32((110.0, 110.0, W / 2, H / 2)), (B, 1))
    depth = raycast_sphere_depth(views, intr, H, W, center, radius)
    return origin, vs, (n, n, n), depth, views, intr, 4 * vs, center, radius
