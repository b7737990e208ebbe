"""Mesh clean-up on the CPU: the torch route of meshclean.py and csrc/meshclean_math.h compiled with g++
(tests/host_math/meshclean_host.cpp visits faces and vertices one after the other), both against the union-find of
tests/meshclean_reference.py on the meshes of tests/test_gpu_meshclean.py; the C-ABI refusals; the export tool's default
bytes; the host build under the address and undefined-behaviour sanitizers as a program of its own.

Everything is integers or gathered floats: every comparison is exact."""
import ctypes
import importlib.util
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import meshclean_reference as M
import tsdf_reference as T

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "host_math" / "meshclean_host.cpp"
LIB = ROOT / "tests" / "host_math" / "libmeshclean_host.so"
HDR = ROOT / "3dgs-deblur_amd" / "csrc" / "meshclean_math.h"
NEW_EXPORTS = {"gs_mesh_clean_workspace_bytes": 2, "gs_mesh_components_round": 7, "gs_mesh_components_finish": 8,
               "gs_mesh_components_table": 9, "gs_mesh_filter_plan": 10, "gs_mesh_filter_emit": 14}
_P, _I = ctypes.c_void_p, ctypes.c_int
EDGE_SIZES = (1, 255, 256, 257, 1023, 1024, 1025)


def P(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def mh():
    if not LIB.exists() or LIB.stat().st_mtime < max(SRC.stat().st_mtime, HDR.stat().st_mtime):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", f"-I{HDR.parent}", str(SRC), "-o", str(LIB)])
    lib = ctypes.CDLL(str(LIB))
    lib.mch_components.argtypes = [_I, _I, _P, _P, _P]
    lib.mch_filter.argtypes = [_I, _I, _P, _P, _P, _I, _I, _P, _P, _P, _P]
    lib.mch_component_key.argtypes = [_I, _I]
    lib.mch_component_key.restype = ctypes.c_ulonglong
    return lib


def host_components(mh, faces, V):
    faces = np.ascontiguousarray(faces, np.int32)
    labels, info = np.zeros(V, np.int32), np.zeros(2, np.int32)
    assert mh.mch_components(V, len(faces), P(faces), P(labels), P(info)) == 0
    return labels, int(info[0]), int(info[1])


def host_filter(mh, verts, faces, colors, min_faces=1, keep_largest=None):
    verts, faces = np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(faces, np.int32)
    colors = None if colors is None else np.ascontiguousarray(colors, np.float32)
    counts = np.zeros(8, np.int32)
    args = (len(verts), len(faces), P(verts), P(faces), P(colors), min_faces, keep_largest or 0, P(counts))
    assert mh.mch_filter(*args, None, None, None) == 0
    vo, fo = np.zeros((counts[0], 3), np.float32), np.zeros((counts[1], 3), np.int32)
    co = None if colors is None else np.zeros((counts[0], 3), np.float32)
    assert mh.mch_filter(*args, P(vo), P(fo), P(co)) == 0
    return vo, fo, co, {"components": int(counts[2]), "kept": int(counts[3])}


def torch_filter(gs, verts, faces, colors, **kw):
    out = gs.mesh_filter_components(torch.from_numpy(verts), torch.from_numpy(faces),
                                    None if colors is None else torch.from_numpy(colors), return_stats=True, **kw)
    assert out[0].dtype == torch.float32 and out[1].dtype == torch.int32
    return out[0].numpy(), out[1].numpy(), None if out[2] is None else out[2].numpy(), out[3]


def same_mesh(got, ref):
    return (np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and got[1].shape == ref[1].shape
            and ((got[2] is None and ref[2] is None) or np.array_equal(got[2], ref[2])))


def check_filter(mh, gs, verts, faces, colors, **kw):
    """the torch route and the host build against the reference -> the reference's result"""
    ref = M.filter_components(verts, faces, colors, **kw)
    tm = torch_filter(gs, verts, faces, colors, **kw)
    assert same_mesh(tm, ref), kw
    assert {k: tm[3][k] for k in ref[3]} == ref[3], (tm[3], ref[3])
    assert 1 <= tm[3]["rounds"] <= gs.meshclean.max_rounds(len(verts))
    if len(verts):
        hm = host_filter(mh, verts, faces, colors, **kw)
        assert same_mesh(hm, ref), kw
        assert hm[3] == {k: ref[3][k] for k in ("components", "kept")}
    return ref


@pytest.fixture(scope="module")
def scene(gs):
    f, main, col = M.scene_fields()
    return tuple(t.numpy() for t in M.scene_mesh(gs, "cpu", f, col)), tuple(t.numpy() for t in M.scene_mesh(gs, "cpu", main, col))


# ---- the header -------------------------------------------------------------------------------------------------------------
def test_header_rules(mh, gs):
    for V in (1, 2, 255, 256, 257, 4097, 2 ** 31 - 1):
        assert mh.mch_max_rounds(V) == 8 * V.bit_length() + 8 == gs.meshclean.max_rounds(V)
    assert mh.mch_max_rounds(257) == 80 and mh.mch_max_rounds(4097) == 112
    assert mh.mch_component_key(5, 7) == (5 << 32) | (0x7fffffff - 7)
    assert mh.mch_component_key(5, 7) > mh.mch_component_key(5, 8) > mh.mch_component_key(4, 0)    # ties: the smaller label
    assert [mh.mch_index_ok(i, 4) for i in (-1, 0, 3, 4, -2 ** 31)] == [0, 1, 1, 0, 0]


# ---- case 1: the scene ------------------------------------------------------------------------------------------------------
def test_scene_oracle(mh, gs, scene):
    (verts, faces, colors), big = scene
    assert (len(verts), len(faces)) == (M.SCENE_V, M.SCENE_F)
    labels, roots, fcount, vcount = (t.numpy() for t in gs.mesh_components(torch.from_numpy(faces), len(verts), return_table=True))
    ref = M.table(faces, len(verts))
    assert all(np.array_equal(a, b) and a.dtype == np.int32 for a, b in zip((labels, roots, fcount, vcount), ref))
    assert tuple(sorted(fcount.tolist(), reverse=True)) == M.SCENE_COMPONENT_FACES and int(vcount.sum()) == len(verts)
    hl, rounds, status = host_components(mh, faces, len(verts))
    assert np.array_equal(hl, labels) and status == 0 and rounds >= 2
    # the largest component IS the main sphere's own mesh, and that is a closed surface of genus 0
    one = check_filter(mh, gs, verts, faces, colors, keep_largest=1)
    assert same_mesh(one, big)
    assert T.is_closed(one[1]) and T.euler(one[0], one[1]) == 2
    for K, F_out in ((2, 7216 + 536), (3, 7216 + 536 + 268), (9, M.SCENE_F)):
        assert len(check_filter(mh, gs, verts, faces, colors, keep_largest=K)[1]) == F_out
    for N, F_out in ((117, 7216 + 536 + 268), (269, 7216 + 536), (537, 7216)):
        assert len(check_filter(mh, gs, verts, faces, colors, min_faces=N)[1]) == F_out
    # the defaults return a mesh whose every vertex is referenced as it came
    assert same_mesh(torch_filter(gs, verts, faces, colors), (verts, faces, colors))
    assert same_mesh(torch_filter(gs, verts, faces, None), (verts, faces, None))


# ---- case 2: rounds ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,random_rounds", [(257, 6), (4097, 8)])
def test_strip_rounds(mh, gs, V, random_rounds):
    verts, _ = M.vertex_data(V)
    for name, numbering in M.numberings(V).items():
        faces = M.strip(V, numbering)
        labels, rounds = gs.meshclean.mesh_components_torch(torch.from_numpy(faces), V, _return_rounds=True)
        assert not labels.any() and labels.dtype == torch.int32, name
        assert rounds == (random_rounds if name == "random" else 2), (name, rounds)      # every side of a round at once
        hl, hrounds, _ = host_components(mh, faces, V)
        assert not hl.any() and 2 <= hrounds <= gs.meshclean.max_rounds(V), (name, hrounds)
    faces = M.interleaved_strips(V)
    labels = gs.mesh_components(torch.from_numpy(faces), 2 * V).numpy()
    assert np.array_equal(labels, np.repeat([0, V], V).astype(np.int32))
    assert np.array_equal(host_components(mh, faces, 2 * V)[0], labels)


# ---- case 3: permutation ------------------------------------------------------------------------------------------------------
def shuffled(verts, faces, colors, seed=7):
    rng = np.random.default_rng(seed)
    order = rng.permutation(len(verts))                 # new vertex n is old vertex order[n]
    inverse = np.empty_like(order)
    inverse[order] = np.arange(len(order))
    faces = inverse[faces][rng.permutation(len(faces))].astype(np.int32)
    return verts[order], faces, colors[order]


def test_shuffled_scene(mh, gs, scene):
    verts, faces, colors = shuffled(*scene[0])
    labels = gs.mesh_components(torch.from_numpy(faces), len(verts)).numpy()
    assert np.array_equal(labels, M.components(faces, len(verts)))
    assert np.array_equal(host_components(mh, faces, len(verts))[0], labels)
    for kw in (dict(keep_largest=1), dict(keep_largest=2, min_faces=537), dict(min_faces=200)):
        check_filter(mh, gs, verts, faces, colors, **kw)


# ---- case 4: edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", EDGE_SIZES)
def test_block_edges(mh, gs, V):
    verts, colors = M.vertex_data(V)
    for F in EDGE_SIZES:
        faces = M.edge_mesh(V, F)
        assert faces.shape == (F, 3)
        labels = gs.mesh_components(torch.from_numpy(faces), V).numpy()
        assert np.array_equal(labels, M.components(faces, V)), (V, F)
        check_filter(mh, gs, verts, faces, colors, keep_largest=2, min_faces=2)


def test_unreferenced_duplicate_and_degenerate(mh, gs):
    V = 12
    faces = np.array([[1, 2, 3], [1, 2, 3], [5, 5, 6], [8, 8, 8], [6, 7, 7], [10, 9, 9]], np.int32)
    verts, colors = M.vertex_data(V)
    labels, roots, fcount, vcount = (t.numpy() for t in gs.mesh_components(torch.from_numpy(faces), V, return_table=True))
    assert labels.tolist() == [0, 1, 1, 1, 4, 5, 5, 5, 8, 9, 9, 11]
    assert roots.tolist() == [0, 1, 4, 5, 8, 9, 11] and fcount.tolist() == [0, 2, 0, 2, 1, 1, 0]
    assert vcount.tolist() == [1, 3, 1, 3, 1, 2, 1]
    assert np.array_equal(host_components(mh, faces, V)[0], labels)
    ref = check_filter(mh, gs, verts, faces, colors)                     # the defaults drop the unreferenced vertices only
    assert len(ref[0]) == 9 and len(ref[1]) == 6 and ref[3]["components"] == 7 and ref[3]["kept"] == 4
    check_filter(mh, gs, verts, faces, colors, min_faces=2)
    check_filter(mh, gs, verts, faces, colors, min_faces=0)              # 0 faces still go
    check_filter(mh, gs, verts, faces, None, keep_largest=3)


def test_tie_goes_to_the_smaller_label(mh, gs):
    faces = np.array([[4, 5, 6], [0, 1, 2], [6, 5, 7], [2, 1, 3]], np.int32)    # two components of two faces each
    verts, colors = M.vertex_data(8)
    ref = check_filter(mh, gs, verts, faces, colors, keep_largest=1)
    assert np.array_equal(ref[0], verts[:4]) and ref[1].tolist() == [[0, 1, 2], [2, 1, 3]]


def test_empty_meshes(gs):
    verts, colors = (torch.from_numpy(a) for a in M.vertex_data(5))
    none = torch.zeros(0, 3, dtype=torch.int32)
    for c in (None, colors):
        v, f, c2, stats = gs.mesh_filter_components(verts, none, c, return_stats=True)
        assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3) and f.dtype == torch.int32 and (c2 is None) == (c is None)
        assert stats == {"components": 5, "kept": 0, "rounds": 0, "verts_in": 5, "faces_in": 0, "verts_out": 0, "faces_out": 0}
    v, f, _ = gs.mesh_filter_components(torch.zeros(0, 3), none)
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3)
    labels, roots, fcount, vcount = gs.mesh_components(none, 5, return_table=True)
    assert labels.tolist() == roots.tolist() == [0, 1, 2, 3, 4] and not fcount.any() and vcount.tolist() == [1] * 5


# ---- case 5: bad input --------------------------------------------------------------------------------------------------------
def test_bad_arguments(mh, gs):
    verts, colors = (torch.from_numpy(a) for a in M.vertex_data(6))
    faces = torch.tensor([[0, 1, 2], [3, 4, 5]], dtype=torch.int32)
    for bad in (-1, 6):
        f = faces.clone()
        f[1, 2] = bad
        with pytest.raises(ValueError, match="outside"):
            gs.mesh_components(f, 6)
        with pytest.raises(ValueError, match="outside"):
            gs.mesh_filter_components(verts, f, colors)
        labels, _, status = host_components(mh, f.numpy(), 6)             # the header skips the face and records it
        assert status == 1 and labels.tolist() == [0, 0, 0, 3, 4, 5]
    for kw in (dict(min_faces=-1), dict(keep_largest=0), dict(keep_largest=-3)):
        with pytest.raises(ValueError):
            gs.mesh_filter_components(verts, faces, colors, **kw)
    with pytest.raises(ValueError):
        gs.mesh_filter_components(verts, faces.long(), colors)
    with pytest.raises(ValueError):
        gs.mesh_filter_components(verts.double(), faces, None)
    with pytest.raises(ValueError):
        gs.mesh_filter_components(verts, faces, colors[:5])
    with pytest.raises(ValueError):
        gs.mesh_filter_components(verts, faces.reshape(3, 2))
    with pytest.raises(ValueError):
        gs.mesh_components(faces, -1)
    with pytest.raises(ValueError, match="no CPU fallback"):
        gs.meshclean.mesh_components_hip(faces, 6)
    with pytest.raises(ValueError, match="no CPU fallback"):
        gs.meshclean.mesh_filter_components_hip(verts, faces, colors)


def test_c_abi_refuses_before_any_launch(gs):
    """null pointers, sizes outside the limits and a short workspace return an error on the host: nothing is launched
    (there is no GPU here)"""
    lib = gs._lib.load()
    for name, n in NEW_EXPORTS.items():
        sig = gs._lib._SIGS.get(name) or gs._lib._SIGS_LL[name]
        assert len(sig) == n, name
    fake, odd = ctypes.c_void_p(256), ctypes.c_void_p(260)
    V, F = 1000, 2000
    need = lib.gs_mesh_clean_workspace_bytes(V, F)
    assert 32 * V + 4 * F <= need < 32 * V + 4 * F + 16 * 256
    assert lib.gs_mesh_clean_workspace_bytes(0, 5) == -1 and lib.gs_mesh_clean_workspace_bytes(5, -1) == -1
    big = 1 << 40
    assert lib.gs_mesh_components_round(V, F, None, None, 0, None, None) == 1
    assert lib.gs_mesh_components_round(V, F, fake, fake, 0, None, None) == 1
    assert lib.gs_mesh_components_round(V, F, None, fake, 0, fake, None) == 1
    assert lib.gs_mesh_components_round(0, F, fake, fake, 0, fake, None) == 1
    assert lib.gs_mesh_components_round(V, F, fake, fake, -1, fake, None) == 1
    assert lib.gs_mesh_components_round(V, F, fake, fake, gs.meshclean.max_rounds(V), fake, None) == 1     # past the guard
    assert lib.gs_mesh_components_finish(V, F, None, None, None, None, 0, None) == 1
    assert lib.gs_mesh_components_finish(V, F, fake, fake, fake, odd, big, None) == 1                      # alignment
    assert lib.gs_mesh_components_finish(V, F, fake, fake, fake, fake, need - 1, None) == 3
    assert lib.gs_mesh_components_table(V, F, 5, None, None, None, None, 0, None) == 1
    assert lib.gs_mesh_components_table(V, F, V + 1, fake, fake, fake, fake, big, None) == 1
    assert lib.gs_mesh_components_table(V, F, 5, fake, fake, fake, fake, need - 1, None) == 3
    assert lib.gs_mesh_components_table(V, F, 5, None, fake, fake, fake, big, None) == 1
    assert lib.gs_mesh_filter_plan(V, F, None, None, 1, 0, None, None, 0, None) == 1
    assert lib.gs_mesh_filter_plan(V, F, fake, fake, -1, 0, fake, fake, big, None) == 1
    assert lib.gs_mesh_filter_plan(V, F, fake, fake, 1, -1, fake, fake, big, None) == 1
    assert lib.gs_mesh_filter_plan(V, 0, fake, fake, 1, 0, fake, fake, big, None) == 1
    assert lib.gs_mesh_filter_plan(V, F, fake, fake, 1, 0, fake, fake, need - 1, None) == 3
    assert lib.gs_mesh_filter_emit(V, F, None, None, None, None, 1, 1, None, None, None, None, 0, None) == 1
    assert lib.gs_mesh_filter_emit(V, F, fake, fake, None, fake, V + 1, 1, fake, fake, None, fake, big, None) == 1
    assert lib.gs_mesh_filter_emit(V, F, fake, fake, fake, fake, 1, 1, fake, fake, None, fake, big, None) == 1   # colours in, none out
    assert lib.gs_mesh_filter_emit(V, F, fake, fake, None, fake, 1, 1, fake, fake, None, fake, need - 1, None) == 3
    assert lib.gs_mesh_filter_emit(V, F, fake, fake, None, fake, 1, 1, None, fake, None, fake, big, None) == 1


# ---- the export tool ----------------------------------------------------------------------------------------------------------
def test_export_tool_default_bytes(gs, scene, tmp_path):
    spec = importlib.util.spec_from_file_location("export_mesh_tool", ROOT / "tools" / "export_mesh.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    verts, faces, colors = (torch.from_numpy(a) for a in scene[0])
    v, f, c, extra = tool.clean_mesh(verts, faces, colors)
    assert v is verts and f is faces and c is colors and extra == {}           # both options off: nothing runs
    gs.tsdf.write_mesh_ply(tmp_path / "plain.ply", verts, faces, colors)
    gs.tsdf.write_mesh_ply(tmp_path / "default.ply", v, f, c)
    assert (tmp_path / "default.ply").read_bytes() == (tmp_path / "plain.ply").read_bytes()
    v, f, c, extra = tool.clean_mesh(verts, faces, colors, keep_largest=1)
    assert extra == {"components": 4, "kept": 1} and same_mesh((v.numpy(), f.numpy(), c.numpy()), scene[1])
    v, f, c, extra = tool.clean_mesh(verts, faces, colors, min_component_faces=269)
    assert extra == {"components": 4, "kept": 2} and len(f) == 7216 + 536
    gs.tsdf.write_mesh_ply(tmp_path / "clean.ply", v, f, c)
    v2, f2, _ = gs.tsdf.read_mesh_ply(tmp_path / "clean.ply")
    assert torch.equal(v2, v) and torch.equal(f2, f)


# ---- sanitizers ---------------------------------------------------------------------------------------------------------------
def test_host_build_under_sanitizers(tmp_path):
    """meshclean_host.cpp as a program of its own (its main runs the small cases) under the address and
    undefined-behaviour sanitizers"""
    exe = tmp_path / "meshclean_host_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DMESHCLEAN_HOST_MAIN", f"-I{HDR.parent}", str(SRC), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "ERROR" not in out.stderr and "runtime error" not in out.stderr
