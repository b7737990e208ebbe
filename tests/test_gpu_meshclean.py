"""Mesh clean-up on the GPU: the kernels of csrc/meshclean.hip against the union-find of tests/meshclean_reference.py and
against gs.tsdf_extract_mesh itself.  Integers and gathered floats only: every comparison is torch.equal / array_equal,
there are no tolerances."""
import numpy as np
import pytest
import torch

import meshclean_reference as M
import tsdf_reference as T

pytestmark = pytest.mark.gpu
EDGE_SIZES = (1, 255, 256, 257, 1023, 1024, 1025)


def gpu_filter(gs, dev, verts, faces, colors, **kw):
    out = gs.mesh_filter_components(torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev),
                                    None if colors is None else torch.from_numpy(colors).to(dev), return_stats=True, **kw)
    assert out[0].dtype == torch.float32 and out[1].dtype == torch.int32 and out[0].device == out[1].device
    assert out[0].is_cuda and tuple(out[0].shape[1:]) == (3,) and tuple(out[1].shape[1:]) == (3,)
    return out[0].cpu().numpy(), out[1].cpu().numpy(), None if out[2] is None else out[2].cpu().numpy(), out[3]


def same_mesh(got, ref):
    return (np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and got[1].shape == ref[1].shape
            and ((got[2] is None and ref[2] is None) or np.array_equal(got[2], ref[2])))


def check_filter(gs, dev, verts, faces, colors, **kw):
    ref = M.filter_components(verts, faces, colors, **kw)
    got = gpu_filter(gs, dev, verts, faces, colors, **kw)
    assert same_mesh(got, ref), kw
    assert {k: got[3][k] for k in ref[3]} == ref[3], (got[3], ref[3])
    assert 1 <= got[3]["rounds"] <= gs.meshclean.max_rounds(len(verts))
    return got


@pytest.fixture(scope="module")
def scene(gs, dev):
    """the five-sphere mesh and the main sphere's own, both from the HIP extraction -> GPU tensors"""
    f, main, col = M.scene_fields()
    return M.scene_mesh(gs, dev, f, col), M.scene_mesh(gs, dev, main, col)


# ---- 1: the oracle that does not depend on the reference ----------------------------------------------------------------
def test_scene_oracle(gs, dev, scene):
    (verts, faces, colors), (bv, bf, bc) = scene
    assert (len(verts), len(faces)) == (M.SCENE_V, M.SCENE_F)
    labels, roots, fcount, vcount = gs.mesh_components(faces, len(verts), return_table=True)
    assert all(t.dtype == torch.int32 and t.is_cuda for t in (labels, roots, fcount, vcount))
    assert tuple(sorted(fcount.tolist(), reverse=True)) == M.SCENE_COMPONENT_FACES and int(vcount.sum()) == len(verts)
    assert roots.tolist() == sorted(roots.tolist()) and torch.equal(labels[roots.long()], roots)
    v1, f1, c1, stats = gs.mesh_filter_components(verts, faces, colors, keep_largest=1, return_stats=True)
    print("scene:", stats)
    assert torch.equal(v1, bv) and torch.equal(f1, bf) and torch.equal(c1, bc)
    assert T.is_closed(f1.cpu().numpy()) and T.euler(v1.cpu().numpy(), f1.cpu().numpy()) == 2
    assert stats == {"components": 4, "kept": 1, "rounds": stats["rounds"], "verts_in": M.SCENE_V, "faces_in": M.SCENE_F,
                     "verts_out": len(bv), "faces_out": 7216}
    assert 2 <= stats["rounds"] <= gs.meshclean.max_rounds(M.SCENE_V)
    vn, fn, cn = (t.cpu().numpy() for t in (verts, faces, colors))
    for K, F_out in ((2, 7216 + 536), (3, 7216 + 536 + 268), (9, M.SCENE_F)):
        assert len(check_filter(gs, dev, vn, fn, cn, keep_largest=K)[1]) == F_out
    for N, F_out in ((117, 7216 + 536 + 268), (269, 7216 + 536), (537, 7216)):
        assert len(check_filter(gs, dev, vn, fn, cn, min_faces=N)[1]) == F_out
    # the defaults give the extraction's mesh back: every vertex of it is referenced
    d = gs.mesh_filter_components(verts, faces, colors)
    assert torch.equal(d[0], verts) and torch.equal(d[1], faces) and torch.equal(d[2], colors)
    d = gs.mesh_filter_components(verts, faces)
    assert torch.equal(d[0], verts) and torch.equal(d[1], faces) and d[2] is None


# ---- 2: rounds ------------------------------------------------------------------------------------------------------------
def test_strip_rounds(gs, dev):
    V = 4097
    verts, colors = M.vertex_data(V)
    for name, numbering in M.numberings(V).items():
        faces = M.strip(V, numbering)
        labels = gs.mesh_components(torch.from_numpy(faces).to(dev), V)
        assert labels.dtype == torch.int32 and tuple(labels.shape) == (V,) and not labels.any(), name
        got = check_filter(gs, dev, verts, faces, colors, keep_largest=1)
        print(f"strip {name}: rounds {got[3]['rounds']}")
        assert got[3]["rounds"] >= 2 and len(got[1]) == V - 2       # the loop iterates: a hooking round, then an empty one
    faces = M.interleaved_strips(V)
    labels = gs.mesh_components(torch.from_numpy(faces).to(dev), 2 * V).cpu().numpy()
    assert np.array_equal(labels, np.repeat([0, V], V).astype(np.int32))


# ---- 3: permutation -------------------------------------------------------------------------------------------------------
def test_shuffled_scene(gs, dev, scene):
    verts, faces, colors = (t.cpu().numpy() for t in scene[0])
    rng = np.random.default_rng(7)
    order = rng.permutation(len(verts))
    inverse = np.empty_like(order)
    inverse[order] = np.arange(len(order))
    faces = inverse[faces][rng.permutation(len(faces))].astype(np.int32)
    verts, colors = verts[order], colors[order]
    labels = gs.mesh_components(torch.from_numpy(faces).to(dev), len(verts)).cpu().numpy()
    assert np.array_equal(labels, M.components(faces, len(verts)))
    for kw in (dict(keep_largest=1), dict(keep_largest=2, min_faces=537), dict(min_faces=200)):
        check_filter(gs, dev, verts, faces, colors, **kw)


# ---- 4: edges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", EDGE_SIZES)
def test_block_edges(gs, dev, V):
    verts, colors = M.vertex_data(V)
    for F in EDGE_SIZES:
        faces = M.edge_mesh(V, F)
        labels, roots, fcount, vcount = (t.cpu().numpy() for t in gs.mesh_components(torch.from_numpy(faces).to(dev), V,
                                                                                     return_table=True))
        assert all(np.array_equal(a, b) for a, b in zip((labels, roots, fcount, vcount), M.table(faces, V))), (V, F)
        check_filter(gs, dev, verts, faces, colors, keep_largest=2, min_faces=2)


def test_unreferenced_duplicate_and_degenerate(gs, dev):
    V = 12
    faces = np.array([[1, 2, 3], [1, 2, 3], [5, 5, 6], [8, 8, 8], [6, 7, 7], [10, 9, 9]], np.int32)
    verts, colors = M.vertex_data(V)
    labels, roots, fcount, vcount = (t.tolist() for t in gs.mesh_components(torch.from_numpy(faces).to(dev), V, return_table=True))
    assert labels == [0, 1, 1, 1, 4, 5, 5, 5, 8, 9, 9, 11]
    assert roots == [0, 1, 4, 5, 8, 9, 11] and fcount == [0, 2, 0, 2, 1, 1, 0] and vcount == [1, 3, 1, 3, 1, 2, 1]
    got = check_filter(gs, dev, verts, faces, colors)
    assert len(got[0]) == 9 and len(got[1]) == 6 and got[3]["components"] == 7 and got[3]["kept"] == 4
    check_filter(gs, dev, verts, faces, colors, min_faces=2)
    check_filter(gs, dev, verts, faces, colors, min_faces=0)
    check_filter(gs, dev, verts, faces, None, keep_largest=3)


def test_tie_goes_to_the_smaller_label(gs, dev):
    faces = np.array([[4, 5, 6], [0, 1, 2], [6, 5, 7], [2, 1, 3]], np.int32)
    verts, colors = M.vertex_data(8)
    got = check_filter(gs, dev, verts, faces, colors, keep_largest=1)
    assert np.array_equal(got[0], verts[:4]) and got[1].tolist() == [[0, 1, 2], [2, 1, 3]]
    # many equal components: exactly K survive, the ones with the smallest labels
    n = 700
    faces = (np.arange(3 * n, dtype=np.int32).reshape(n, 3))[np.random.default_rng(4).permutation(n)]
    verts, colors = M.vertex_data(3 * n)
    got = check_filter(gs, dev, verts, faces, colors, keep_largest=300)
    assert np.array_equal(got[0], verts[:900]) and got[3]["kept"] == 300


def test_no_faces(gs, dev):
    verts, colors = (torch.from_numpy(a).to(dev) for a in M.vertex_data(5))
    none = torch.zeros(0, 3, dtype=torch.int32, device=dev)
    v, f, c, stats = gs.mesh_filter_components(verts, none, colors, return_stats=True)
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3) and tuple(c.shape) == (0, 3) and v.is_cuda
    assert stats == {"components": 5, "kept": 0, "rounds": 0, "verts_in": 5, "faces_in": 0, "verts_out": 0, "faces_out": 0}
    assert gs.mesh_components(none, 5).tolist() == [0, 1, 2, 3, 4]


# ---- 5: bad input ---------------------------------------------------------------------------------------------------------
def test_bad_face_index_is_a_value_error(gs, dev):
    """the kernels test every index before they use it and leave a status word: a guarded read, no address is formed"""
    V = 600
    faces = M.strip(V)
    verts, colors = M.vertex_data(V)
    for bad in (-1, V):
        f = faces.copy()
        f[311, 1] = bad
        with pytest.raises(ValueError, match="outside"):
            gs.mesh_components(torch.from_numpy(f).to(dev), V)
        with pytest.raises(ValueError, match="outside"):
            gs.mesh_filter_components(torch.from_numpy(verts).to(dev), torch.from_numpy(f).to(dev))
        check_filter(gs, dev, verts, faces, colors, keep_largest=1)          # the same process's next call succeeds


# ---- 6: determinism -------------------------------------------------------------------------------------------------------
def test_runs_agree_and_match_the_cpu_route(gs, dev, scene):
    verts, faces, colors = scene[0]
    cpu = tuple(t.cpu() for t in scene[0])
    for kw in (dict(keep_largest=1), dict(keep_largest=3), dict(min_faces=269), dict()):
        a = gs.mesh_filter_components(verts, faces, colors, **kw)
        b = gs.mesh_filter_components(verts, faces, colors, **kw)
        c = gs.mesh_filter_components(*cpu, **kw)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), kw
        assert all(torch.equal(x.cpu(), y) for x, y in zip(a, c)), kw
    t1 = gs.mesh_components(faces, len(verts), return_table=True)
    t2 = gs.mesh_components(faces, len(verts), return_table=True)
    t3 = gs.mesh_components(cpu[1], len(verts), return_table=True)
    assert all(torch.equal(x, y) and torch.equal(x.cpu(), z) for x, y, z in zip(t1, t2, t3))
