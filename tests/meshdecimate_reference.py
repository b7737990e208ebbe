"""TEST INFRASTRUCTURE ONLY: mesh decimation by vertex clustering in numpy float64, written from the rule's text (the
docstring of gsdeblur_amd/meshdecimate.py) and not from csrc/meshdecimate_math.h: np.unique on the cell triples, a dict for
the dedupe, np.linalg.solve for the 3x3 system, and the same bisection over the ladder of cell sizes.  Also the meshes the
host and the GPU tests share, and the comparison rule."""
import numpy as np

LADDER = 64


class Refused(ValueError):
    pass


def plan(verts, faces, s, dedupe=True):
    verts, faces = np.asarray(verts, np.float32), np.asarray(faces, np.int32)
    V = len(verts)
    with np.errstate(all="ignore"):
        q = verts.astype(np.float64) / float(s)
    if not np.isfinite(q).all():
        raise Refused("vertex")
    cells = np.floor(q)
    if (np.abs(cells) > 2.0 ** 30).any():
        raise Refused("vertex")
    if len(faces) and (faces.min() < 0 or faces.max() >= V):
        raise Refused("face")
    cells = cells.astype(np.int64)
    unique, cluster = np.unique(cells[:, ::-1], axis=0, return_inverse=True)        # rows (cz, cy, cx), ascending
    cluster = cluster.reshape(-1)
    tri = cluster[faces]
    keep, seen = np.zeros(len(faces), bool), {}
    degenerate = duplicates = 0
    for f, (a, b, c) in enumerate(tri.tolist()):
        if a == b or b == c or a == c:
            degenerate += 1
            continue
        key = tuple(sorted((a, b, c)))
        if dedupe and key in seen:
            duplicates += 1
            continue
        seen[key] = f
        keep[f] = True
    ref = np.zeros(len(unique), bool)
    ref[tri[keep].reshape(-1)] = True
    return dict(s=float(s), cells=unique[:, ::-1], cluster=cluster, tri=tri, keep=keep, ref=ref, degenerate=degenerate,
                duplicates=duplicates, faces_out=int(keep.sum()), verts_out=int(ref.sum()), clusters=len(unique))


def emit(verts, faces, colors, p):
    verts, faces = np.asarray(verts, np.float32).astype(np.float64), np.asarray(faces, np.int32)
    s, cluster, C = p["s"], p["cluster"], p["clusters"]
    centre = (p["cells"].astype(np.float64) + 0.5) * s
    count = np.bincount(cluster, minlength=C).astype(np.float64)[:, None]
    m = np.zeros((C, 3))
    np.add.at(m, cluster, verts - centre[cluster])              # unbuffered: one member after the other
    m /= count
    A, b = np.zeros((C, 3, 3)), np.zeros((C, 3))
    for k in range(3):                                          # every (face, corner): the corner's cluster gets the plane
        c = cluster[faces[:, k]]
        p0, p1, p2 = (verts[faces[:, j]] - centre[c] for j in range(3))
        n = np.cross(p1 - p0, p2 - p0)
        d = -np.einsum("ij,ij->i", n, p0)
        np.add.at(A, c, n[:, :, None] * n[:, None, :])
        np.add.at(b, c, d[:, None] * n)
    tr = np.trace(A, axis1=1, axis2=2)
    y = np.zeros((C, 3))
    ok = np.isfinite(tr) & (tr != 0)
    if ok.any():
        y[ok] = np.linalg.solve(A[ok] + 1e-3 * tr[ok, None, None] * np.eye(3), -(b[ok] + np.einsum("cij,cj->ci", A[ok], m[ok]))[:, :, None])[:, :, 0]
    out = centre + np.clip(m + y, -0.5 * s, 0.5 * s)
    ref = p["ref"]
    new_index = np.cumsum(ref) - 1
    verts_out = out[ref].astype(np.float32)
    colors_out = None
    if colors is not None:
        csum = np.zeros((C, 3))
        np.add.at(csum, cluster, np.asarray(colors, np.float32).astype(np.float64))
        colors_out = (csum / count)[ref].astype(np.float32)
    faces_out = new_index[p["tri"][p["keep"]]].astype(np.int32).reshape(-1, 3)
    cluster_of = np.where(ref[cluster], new_index[cluster], -1).astype(np.int32)
    return verts_out, faces_out, colors_out, cluster_of


def choose(reaches):
    if reaches(0):
        return 0
    if not reaches(LADDER - 1):
        raise Refused("target")
    lo, hi = 0, LADDER - 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if reaches(mid):
            hi = mid
        else:
            lo = mid
    return hi


def decimate(verts, faces, colors=None, cell_size=None, target_faces=None, dedupe=True):
    """-> (verts', faces', colors', cluster_of, stats); stats as gs.mesh_decimate's plus `index`, the ladder index used"""
    plans = {}

    def at(i):
        if i not in plans:
            plans[i] = plan(verts, faces, float(cell_size) * 2.0 ** (i / 4), dedupe)
        return plans[i]
    index = 0 if target_faces is None else choose(lambda i: at(i)["faces_out"] <= target_faces)
    p = at(index)
    v, f, c, m = emit(verts, faces, colors, p)
    stats = {"cell_size": p["s"], "plans": len(plans), "clusters": p["clusters"], "verts_in": len(verts), "faces_in": len(faces),
             "verts_out": p["verts_out"], "faces_out": p["faces_out"], "degenerate": p["degenerate"],
             "duplicates": p["duplicates"], "index": index}
    return v, f, c, m, stats


# ---- the comparison rule ------------------------------------------------------------------------------------------------------
def ulp_error(got, ref, floor):
    """the largest |got - ref| in float32 ulps of max(|ref|, floor) (0.0 for empty arrays)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.size == 0:
        return 0.0
    scale = np.maximum(np.abs(ref), floor).astype(np.float32)
    return float((np.abs(got - ref) / np.spacing(scale).astype(np.float64)).max())


def assert_same(got, ref, s, what=""):
    """got, ref: (verts', faces', colors', cluster_of, stats).  Every integer equal; positions within 2 float32 ulps of
    max(|coordinate|, s), colours within 2 ulps of max(|value|, s): the float64 solutions agree to about
    1e-12 (condition number about 1e3), so the only visible difference is a flipped final rounding to float32 — one ulp —
    and the second ulp is margin."""
    assert got[1].shape == ref[1].shape and np.array_equal(got[1], ref[1]), what
    assert np.array_equal(got[3], ref[3]), what
    assert {k: got[4][k] for k in ref[4] if k != "index"} == {k: v for k, v in ref[4].items() if k != "index"}, (what, got[4], ref[4])
    assert got[0].shape == ref[0].shape and got[0].dtype == np.float32, what
    err = ulp_error(got[0], ref[0], s)
    print(f"{what}: positions differ by {err:.2f} ulp at most")
    assert err <= 2.0, (what, err)
    assert (got[2] is None) == (ref[2] is None), what
    if ref[2] is not None:
        cerr = ulp_error(got[2], ref[2], s)
        assert got[2].shape == ref[2].shape and cerr <= 2.0, (what, cerr)


# ---- the meshes ---------------------------------------------------------------------------------------------------------------
EDGE_SIZES = ((1, 255), (255, 1), (256, 257), (257, 256), (1023, 1025), (1025, 1023))


def cube_soup():
    """the unit cube as 12 triangles with no shared vertex -> verts [36,3], faces [12,3]"""
    quads = [((0, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 0)), ((0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)),
             ((0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1)), ((0, 1, 0), (0, 1, 1), (1, 1, 1), (1, 1, 0)),
             ((0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0)), ((1, 0, 0), (1, 1, 0), (1, 1, 1), (1, 0, 1))]
    verts = []
    for a, b, c, d in quads:
        verts += [a, b, c, a, c, d]
    return np.array(verts, np.float32), np.arange(36, dtype=np.int32).reshape(12, 3)


def plane(n=32):
    """vertices (i, j, 0), 0 <= i, j <= n, two triangles per square"""
    j, i = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    verts = np.stack([i.reshape(-1), j.reshape(-1), np.zeros((n + 1) ** 2)], 1).astype(np.float32)
    a = (j[:-1, :-1] * (n + 1) + i[:-1, :-1]).reshape(-1)
    faces = np.concatenate([np.stack([a, a + 1, a + n + 2], 1), np.stack([a, a + n + 2, a + n + 1], 1)]).astype(np.int32)
    return verts, faces


def tetrahedron():
    verts = np.array([[0.1, 0.1, 0.1], [0.4, 0.1, 0.1], [0.1, 0.4, 0.1], [0.1, 0.1, 0.4]], np.float32)
    return verts, np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)


def octant_faces():
    """two faces whose corners lie in three octants: the corners never share a cell whatever the cell size, so a face
    always survives; at s = 1 both do, from s = 4 the second is a duplicate of the first"""
    verts = np.array([[-1, -1, -1], [1, -1, -1], [-1, 1, -1], [-3, -3, -3], [3, -3, -3], [-3, 3, -3]], np.float32)
    return verts, np.array([[0, 1, 2], [3, 4, 5]], np.int32)


def soup(V, F, seed=0):
    """a random soup in [-3, 3]^3 for s = 0.5: some coordinates exactly on multiples of s, negatives, -0.0; faces drawn with
    repeats, both orientations of some triples and some repeated corners -> verts, faces, colors"""
    rng = np.random.default_rng(1000 * V + F + seed)
    verts = rng.uniform(-3, 3, (V, 3)).astype(np.float32)
    on_grid = rng.random((V, 3)) < 0.2
    verts[on_grid] = (rng.integers(-6, 7, (V, 3)).astype(np.float32) * 0.5)[on_grid]
    verts[rng.random((V, 3)) < 0.03] = -0.0
    faces = rng.integers(0, V, (F, 3)).astype(np.int32)
    for f in range(1, F):
        r = rng.random()
        if r < 0.15:
            faces[f] = faces[rng.integers(0, f)]                     # a repeat
        elif r < 0.3:
            faces[f] = faces[rng.integers(0, f)][::-1]               # the other orientation
        elif r < 0.4:
            faces[f, 1] = faces[f, 0]                                # a repeated corner
    colors = rng.random((V, 3)).astype(np.float32)
    return verts, faces, colors


def edge_counts(faces):
    """-> {number of faces on an edge: edges with that number}"""
    e = np.sort(np.concatenate([faces[:, (0, 1)], faces[:, (1, 2)], faces[:, (2, 0)]]), axis=1)
    _, n = np.unique(e, axis=0, return_counts=True)
    return {int(k): int((n == k).sum()) for k in np.unique(n)}


def is_closed_genus0(verts, faces):
    counts = edge_counts(faces)
    edges = sum(counts.values())
    return set(counts) == {2} and len(verts) - edges + len(faces) == 2
