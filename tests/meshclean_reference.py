"""Reference for the mesh clean-up tests (tests/test_meshclean_host.py, tests/test_gpu_meshclean.py): a plain union-find
written from the rule, sharing no code with the product, and the meshes both test files use.

The rule: the vertices are nodes, the three sides of every face edges; labels[v] is the smallest vertex index of v's
component; a face belongs to the component of its vertices.  Filter: rank the components with at least one face by (face
count descending, label ascending); keep_largest = K keeps the first min(K, C) of them; of those the ones with fewer than
min_faces faces go; components without a face always go; what stays keeps its order, faces are re-indexed."""
import functools

import numpy as np

import tsdf_reference as T


def components(faces, V):
    """-> labels [V] int32 by union-find (union under the smaller root, path halving)"""
    parent = list(range(V))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v
    for a, b, c in np.asarray(faces).reshape(-1, 3).tolist():
        for p, q in ((a, b), (b, c), (c, a)):
            rp, rq = find(p), find(q)
            if rp != rq:
                parent[max(rp, rq)] = min(rp, rq)
    return np.array([find(v) for v in range(V)], np.int32)


def table(faces, V):
    """-> (labels, roots ascending, face counts, vertex counts)"""
    labels = components(faces, V)
    roots = sorted(set(labels.tolist()))
    fcount = {r: 0 for r in roots}
    vcount = {r: 0 for r in roots}
    for v in range(V):
        vcount[int(labels[v])] += 1
    for a, _, _ in np.asarray(faces).reshape(-1, 3).tolist():
        fcount[int(labels[a])] += 1
    return (labels, np.array(roots, np.int32), np.array([fcount[r] for r in roots], np.int32),
            np.array([vcount[r] for r in roots], np.int32))


def filter_components(verts, faces, colors=None, min_faces=1, keep_largest=None):
    """-> (verts', faces', colors', stats without rounds)"""
    verts, faces = np.asarray(verts), np.asarray(faces).reshape(-1, 3)
    V, F = len(verts), len(faces)
    labels, roots, fcount, _ = table(faces, V)
    count_of = dict(zip(roots.tolist(), fcount.tolist()))
    ranked = sorted((r for r in roots.tolist() if count_of[r] >= 1), key=lambda r: (-count_of[r], r))
    if keep_largest is not None:
        ranked = ranked[:keep_largest]
    survivors = {r for r in ranked if count_of[r] >= min_faces}
    keep_v = np.array([int(labels[v]) in survivors for v in range(V)], bool)
    new = np.full(V, -1, np.int64)
    new[keep_v] = np.arange(int(keep_v.sum()))
    keep_f = keep_v[faces[:, 0]] if F else np.zeros(0, bool)
    faces_out = new[faces[keep_f]].astype(np.int32).reshape(-1, 3)
    stats = {"components": len(roots), "kept": len(survivors), "verts_in": V, "faces_in": F,
             "verts_out": int(keep_v.sum()), "faces_out": int(keep_f.sum())}
    return verts[keep_v], faces_out, None if colors is None else np.asarray(colors)[keep_v], stats


# ---- meshes ---------------------------------------------------------------------------------------------------------------
SCENE_N = 32
MAIN_SPHERE = ((16.63, 17.41, 19.27), 8.0)
FLOATERS = (((5.3, 6.6, 7.2), 1.6), ((28.2, 7.1, 9.4), 2.2), ((6.5, 28.7, 29.1), 1.2), ((27.5, 28.5, 7.5), 0.8))
SCENE_V, SCENE_F = 4076, 8136                        # the CPU extraction of the scene
SCENE_COMPONENT_FACES = (7216, 536, 268, 116)        # the radius-0.8 floater crosses no sample and leaves nothing


@functools.lru_cache(maxsize=None)
def scene_fields():
    """-> (the minimum of the five sphere fields, the main sphere's field alone, the colours), float32 [32,32,32(,3)]"""
    main = T.sphere_field(SCENE_N, *MAIN_SPHERE)
    f = main
    for c, r in FLOATERS:
        f = np.minimum(f, T.sphere_field(SCENE_N, c, r))
    return f, main, T.field_colors(f.shape)


def scene_mesh(gs, device, field, colors):
    """gs.tsdf_extract_mesh of a 32^3 volume (origin tsdf_reference.MESH_ORIGIN, voxel 1, weight 1) on `device`"""
    import torch
    vol = gs.TSDFVolume(T.MESH_ORIGIN, 1.0, (SCENE_N,) * 3, device=device)
    vol.tsdf.copy_(torch.from_numpy(field))
    vol.weight.fill_(1.0)
    vol.color.copy_(torch.from_numpy(colors))
    return gs.tsdf_extract_mesh(vol)


def strip(V, numbering=None, offset=0):
    """the triangle strip (i, i+1, i+2) of V vertices -> faces [V-2,3] int32, vertex i named numbering[i] + offset"""
    i = np.arange(max(V - 2, 0))
    f = np.stack([i, i + 1, i + 2], axis=1)
    if numbering is not None:
        f = np.asarray(numbering)[f]
    return (f + offset).astype(np.int32)


def numberings(V):
    return {"identity": np.arange(V), "reversed": np.arange(V)[::-1].copy(),
            "random": np.random.default_rng(0).permutation(V)}


def interleaved_strips(V):
    """two random-numbered strips of V vertices each, the second on vertices V .. 2V-1, faces alternating"""
    a = strip(V, np.random.default_rng(1).permutation(V))
    b = strip(V, np.random.default_rng(2).permutation(V), offset=V)
    f = np.empty((2 * len(a), 3), np.int32)
    f[0::2], f[1::2] = a, b
    return f


def edge_mesh(V, F):
    """exactly V vertices and F faces for the block-edge cases: a strip over the first vertices, isolated triangles behind
    it while vertices and faces last, then duplicates of the last face; vertices left over are unreferenced"""
    faces = []
    s = min(V, max(3, V // 2)) if V >= 3 else 0
    faces += strip(s).tolist()[:F]
    at = s
    while len(faces) < F and at + 3 <= V:
        faces.append([at, at + 1, at + 2])
        at += 3
    if V < 3:
        faces = [[0, 0, V - 1]] * min(F, 1)            # only degenerate faces fit
    while len(faces) < F:
        faces.append(list(faces[-1]))
    return np.array(faces, np.int32).reshape(-1, 3)


def vertex_data(V, seed=3):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((V, 3)).astype(np.float32), rng.random((V, 3)).astype(np.float32)
