"""Mesh decimation on the CPU: the torch route of meshdecimate.py and csrc/meshdecimate_math.h compiled with g++
(tests/host_math/meshdecimate_host.cpp), both against the numpy reference of tests/meshdecimate_reference.py on the meshes
of tests/test_gpu_meshdecimate.py; the descriptor's ctypes mirror against the header; the C-ABI refusals; argument
validation; the export tool's bytes; the host build under the address and undefined-behaviour sanitizers as a program of
its own.

Comparison (meshdecimate_reference.assert_same): every integer equal; positions and colours within 2 float32 ulps of
max(|value|, s) — derived there, not measured.  No case is excluded."""
import ctypes
import importlib.util
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import meshclean_reference as M
import meshdecimate_reference as R

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "host_math" / "meshdecimate_host.cpp"
LIB = ROOT / "tests" / "host_math" / "libmeshdecimate_host.so"
HDR = ROOT / "3dgs-deblur_amd" / "csrc" / "meshdecimate_math.h"
_P, _I, _D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double


def P(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def mh():
    if not LIB.exists() or LIB.stat().st_mtime < max(SRC.stat().st_mtime, HDR.stat().st_mtime):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", f"-I{HDR.parent}", str(SRC),
                               "-o", str(LIB)])
    lib = ctypes.CDLL(str(LIB))
    lib.mdh_decimate.argtypes = [_I, _I, _P, _P, _P, _D, _I, _P, _P, _P, _P, _P]
    lib.mdh_cell_of.argtypes = [ctypes.c_float, _D, _P]
    return lib


def host_decimate(mh, verts, faces, colors, s, dedupe=True):
    """the host build of the header -> (verts', faces', colors', cluster_of, stats without cell_size and plans)"""
    verts, faces = np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(faces, np.int32)
    colors = None if colors is None else np.ascontiguousarray(colors, np.float32)
    counts = np.zeros(8, np.int32)
    args = (len(verts), len(faces), P(verts), P(faces), P(colors), float(s), 1 if dedupe else 0, P(counts))
    assert mh.mdh_decimate(*args, None, None, None, None) == 0
    if counts[5]:
        raise R.Refused({1: "face", 2: "vertex"}[int(counts[5])])
    # one spare row each: a NULL verts_out means "count only", and an empty array has no address worth passing
    vo, fo = np.zeros((counts[0] + 1, 3), np.float32), np.zeros((counts[1] + 1, 3), np.int32)
    co = None if colors is None else np.zeros((counts[0] + 1, 3), np.float32)
    cluster_of = np.zeros(len(verts), np.int32)
    assert mh.mdh_decimate(*args, P(vo), P(fo), P(co), P(cluster_of)) == 0
    vo, fo, co = vo[:-1], fo[:-1], None if co is None else co[:-1]
    stats = {"clusters": int(counts[2]), "verts_in": len(verts), "faces_in": len(faces), "verts_out": int(counts[0]),
             "faces_out": int(counts[1]), "degenerate": int(counts[3]), "duplicates": int(counts[4])}
    return vo, fo, co, cluster_of, stats


def torch_decimate(gs, verts, faces, colors, s, **kw):
    out = gs.mesh_decimate(torch.from_numpy(verts), torch.from_numpy(faces), None if colors is None else torch.from_numpy(colors),
                           cell_size=s, return_map=True, return_stats=True, **kw)
    assert out[0].dtype == torch.float32 and out[1].dtype == torch.int32 and out[3].dtype == torch.int32
    return out[0].numpy(), out[1].numpy(), None if out[2] is None else out[2].numpy(), out[3].numpy(), out[4]


def check(mh, gs, verts, faces, colors, s, what, **kw):
    """the torch route and the host build against the reference -> the reference's result"""
    ref = R.decimate(verts, faces, colors, s, **kw)
    R.assert_same(torch_decimate(gs, verts, faces, colors, s, **kw), ref, ref[4]["cell_size"], what + " torch")
    host = host_decimate(mh, verts, faces, colors, ref[4]["cell_size"], kw.get("dedupe", True))
    sub = ref[:4] + ({k: ref[4][k] for k in host[4]},)
    R.assert_same(host, sub, ref[4]["cell_size"], what + " host")
    return ref


@pytest.fixture(scope="module")
def sphere(gs):
    """the main sphere of the clean-up tests' scene, extracted at 32^3 with voxel 1 (7216 faces, closed)"""
    _, main, col = M.scene_fields()
    return tuple(t.numpy() for t in M.scene_mesh(gs, "cpu", main, col))


# ---- the header -------------------------------------------------------------------------------------------------------------
def test_cell_rule(mh):
    c = ctypes.c_int(7)
    for v, s, want in ((0.0, 0.5, 0), (-0.0, 0.5, 0), (0.5, 0.5, 1), (-0.5, 0.5, -1), (-0.25, 0.5, -1), (0.49999997, 0.5, 0),
                       (-1e-30, 0.5, -1), (2.0 ** 30, 1.0, 2 ** 30), (-2.0 ** 30, 1.0, -2 ** 30), (3.0, 0.125, 24)):
        assert mh.mdh_cell_of(v, s, ctypes.byref(c)) == 1 and c.value == want, (v, s, c.value)
        assert c.value == int(np.floor(np.float64(np.float32(v)) / s))
    for v, s in ((float("nan"), 1.0), (float("inf"), 1.0), (-float("inf"), 1.0), (1e30, 0.5), (2.0 ** 30 + 128, 1.0),
                 (-2.0 ** 30 - 128, 1.0), (1.0, 1e-10)):
        assert mh.mdh_cell_of(v, s, ctypes.byref(c)) == 0 and c.value == 0, (v, s)
    assert [mh.mdh_index_bits(n) for n in (1, 2, 3, 256, 257, 2 ** 21, 2 ** 30)] == [1, 1, 2, 8, 9, 21, 30]


# ---- the meshes of the GPU tests ----------------------------------------------------------------------------------------------
def test_weld(mh, gs):
    verts, faces = R.cube_soup()
    ref = check(mh, gs, verts, faces, None, 0.125, "cube")
    assert ref[4]["verts_out"] == 8 and ref[4]["faces_out"] == 12 and ref[4]["clusters"] == 8
    # three planes meet at a corner: the quadric puts the representative there
    assert R.ulp_error(ref[0][ref[3]], verts, 0.125) <= 2.0


def test_plane(mh, gs):
    verts, faces = R.plane(32)
    ref = check(mh, gs, verts, faces, None, 2.0, "plane")
    assert ref[4]["clusters"] == 17 * 17 == ref[4]["verts_out"]
    assert not ref[0][:, 2].any()
    cluster = ref[3]
    means = np.stack([verts[cluster == c].astype(np.float64).mean(0) for c in range(289)])
    assert R.ulp_error(ref[0][:, :2], means[:, :2], 2.0) <= 2.0
    out = torch_decimate(gs, verts, faces, None, 2.0)
    assert not out[0][:, 2].any() and not host_decimate(mh, verts, faces, None, 2.0)[0][:, 2].any()


def test_everything_collapses(mh, gs):
    verts, faces = R.tetrahedron()
    ref = check(mh, gs, verts, faces, None, 1.0, "tetrahedron")
    assert ref[0].shape == (0, 3) and ref[1].shape == (0, 3) and ref[4]["degenerate"] == 4 and (ref[3] == -1).all()


@pytest.mark.parametrize("V,F", R.EDGE_SIZES)
def test_block_edges(mh, gs, V, F):
    verts, faces, colors = R.soup(V, F)
    assert (verts == 0.5).any() or V < 8
    for dedupe in (True, False):
        ref = check(mh, gs, verts, faces, colors, 0.5, f"soup {V} {F} dedupe {dedupe}", dedupe=dedupe)
        assert ref[4]["faces_out"] + ref[4]["degenerate"] + ref[4]["duplicates"] == F
        assert dedupe or ref[4]["duplicates"] == 0


def test_sphere(mh, gs, sphere):
    verts, faces, colors = sphere
    closed = []
    for s in (2.0, 1.5, 3.0):
        ref = check(mh, gs, verts, faces, colors, s, f"sphere {s}")
        closed.append(R.is_closed_genus0(ref[0], ref[1]))
        print(f"sphere s = {s}: F' {len(ref[1])}, edge uses {R.edge_counts(ref[1])}, closed genus 0: {closed[-1]}")
        assert len(ref[1]) < len(faces)


def test_target_faces(mh, gs, sphere):
    verts, faces, colors = sphere
    for N in (len(faces) // 4, len(faces) // 20, len(faces)):
        ref = R.decimate(verts, faces, colors, 1.0, target_faces=N)
        got = torch_decimate(gs, verts, faces, colors, 1.0, target_faces=N)
        R.assert_same(got, ref, ref[4]["cell_size"], f"target {N}")
        assert got[4]["faces_out"] <= N and got[4]["cell_size"] == 2.0 ** (ref[4]["index"] / 4) and got[4]["plans"] <= 8
        assert (ref[4]["index"] == 0) == (N == len(faces))
        host = host_decimate(mh, verts, faces, colors, ref[4]["cell_size"])
        R.assert_same(host, ref[:4] + ({k: ref[4][k] for k in host[4]},), ref[4]["cell_size"], f"target {N} host")
    # corners in three octants never share a cell: one face always survives, N = 0 is not reached
    v, f = R.octant_faces()
    got = torch_decimate(gs, v, f, None, 1.0, target_faces=1)
    assert got[4]["faces_out"] == 1 and got[4]["duplicates"] == 1 and got[4]["cell_size"] > 1.0
    R.assert_same(got, R.decimate(v, f, None, 1.0, target_faces=1), got[4]["cell_size"], "octants")
    with pytest.raises(ValueError, match="not reached"):
        torch_decimate(gs, v, f, None, 1.0, target_faces=0)
    with pytest.raises(R.Refused):
        R.decimate(v, f, None, 1.0, target_faces=0)


# ---- bad input ----------------------------------------------------------------------------------------------------------------
def test_refusals(mh, gs):
    verts, faces, colors = R.soup(257, 256)
    for bad in (-1, 257):
        f = faces.copy()
        f[100, 1] = bad
        with pytest.raises(ValueError, match="outside"):
            torch_decimate(gs, verts, f, colors, 0.5)
        with pytest.raises(R.Refused, match="face"):
            host_decimate(mh, verts, f, colors, 0.5)
    for bad in (float("nan"), float("inf"), 1e30):
        v = verts.copy()
        v[77, 2] = bad
        with pytest.raises(ValueError, match="not finite or more than"):
            torch_decimate(gs, v, faces, colors, 0.5)
        with pytest.raises(R.Refused, match="vertex"):
            host_decimate(mh, v, faces, colors, 0.5)
        with pytest.raises(R.Refused, match="vertex"):
            R.decimate(v, faces, colors, 0.5)


def test_bad_arguments(gs):
    verts, faces, colors = (torch.from_numpy(a) for a in R.soup(16, 8))
    with pytest.raises(ValueError, match="cell_size is required"):
        gs.mesh_decimate(verts, faces, colors)
    for s in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cell_size"):
            gs.mesh_decimate(verts, faces, colors, cell_size=s)
    for N in (-1, 2.5, True):
        with pytest.raises(ValueError, match="target_faces"):
            gs.mesh_decimate(verts, faces, colors, cell_size=0.5, target_faces=N)
    with pytest.raises(ValueError):
        gs.mesh_decimate(verts, faces.long(), colors, cell_size=0.5)
    with pytest.raises(ValueError):
        gs.mesh_decimate(verts.double(), faces, None, cell_size=0.5)
    with pytest.raises(ValueError):
        gs.mesh_decimate(verts, faces, colors[:5], cell_size=0.5)
    with pytest.raises(ValueError):
        gs.mesh_decimate(verts, faces.reshape(12, 2), cell_size=0.5)
    with pytest.raises(ValueError, match="no CPU fallback"):
        gs.meshdecimate.mesh_decimate_hip(verts, faces, colors, cell_size=0.5)


def test_empty_meshes(gs):
    verts, _, colors = (torch.from_numpy(a) for a in R.soup(5, 1))
    none = torch.zeros(0, 3, dtype=torch.int32)
    for c in (None, colors):
        v, f, c2, cluster_of, stats = gs.mesh_decimate(verts, none, c, cell_size=0.5, return_map=True, return_stats=True)
        assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3) and f.dtype == torch.int32 and (c2 is None) == (c is None)
        assert cluster_of.tolist() == [-1] * 5 and cluster_of.dtype == torch.int32
        assert stats == {"cell_size": 0.5, "plans": 0, "clusters": 0, "verts_in": 5, "faces_in": 0, "verts_out": 0,
                         "faces_out": 0, "degenerate": 0, "duplicates": 0}
    out = gs.mesh_decimate(torch.zeros(0, 3), none, cell_size=0.5, target_faces=10)
    assert len(out) == 3 and tuple(out[0].shape) == (0, 3)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_descriptor_matches_the_header_layout(gs, tmp_path):
    """the ctypes mirror of gs_mesh_decimate_desc against the C header itself (gcc prints sizeof and every offsetof), and the
    header has no member the mirror lacks; the stream is the last field"""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    cls, cname = gs.meshdecimate._Desc, "gs_mesh_decimate_desc"
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT / "include" / "gsdeblur.h"}"', 'int main(void) {',
             f'  printf("{cname} %zu\\n", sizeof({cname}));']
    lines += [f'  printf("{name} %zu\\n", offsetof({cname}, {name}));' for name, _ in cls._fields_]
    lines += ['  return 0;', '}']
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")])
    got = dict(ln.split() for ln in subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines())
    assert int(got[cname]) == ctypes.sizeof(cls)
    for name, _ in cls._fields_:
        assert int(got[name]) == getattr(cls, name).offset, name
    hdr = (ROOT / "include" / "gsdeblur.h").read_text()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [d.strip() for decl in body.split(";") if decl.strip() for d in decl.split(",")]
    assert len(members) == len(cls._fields_)
    assert cls._fields_[-1][0] == "stream" and re.fullmatch(r"void\s*\*\s*stream", members[-1])


def test_c_abi_refuses_before_any_launch(gs):
    """null pointers, sizes outside the limits, a bad cell size and a short workspace return an error on the host: nothing is
    launched (there is no GPU here)"""
    lib = gs._lib.load()
    assert gs._lib._SIGS["gs_mesh_decimate_plan"] == [_P] == gs._lib._SIGS["gs_mesh_decimate_emit"]
    assert len(gs._lib._SIGS_LL["gs_mesh_decimate_workspace_bytes"]) == 2
    V, F = 1000, 2000
    need = lib.gs_mesh_decimate_workspace_bytes(V, F)
    assert need > 48 * V + 20 * F
    for bad in ((0, 5), (5, 0), (-1, 5), (5, -1), (2 ** 30 + 1, 5), (5, (2 ** 31 - 1) // 3 + 1), (5, 2 ** 30)):
        assert lib.gs_mesh_decimate_workspace_bytes(*bad) == -1, bad
    assert lib.gs_mesh_decimate_workspace_bytes(2 ** 30, (2 ** 31 - 1) // 3) > 2 ** 36          # the limits themselves: 3 F fits an int

    def desc(**kw):
        d = gs.meshdecimate._Desc()
        d.V, d.F, d.verts, d.faces, d.cell_size, d.dedupe, d.counts, d.ws, d.ws_bytes = V, F, 256, 256, 0.5, 1, 256, 256, 1 << 40
        d.verts_out, d.faces_out, d.V_out, d.F_out = 256, 256, 1, 1
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def call(fn, d):
        return fn(ctypes.c_void_p(ctypes.addressof(d)) if d is not None else None)
    for fn in (lib.gs_mesh_decimate_plan, lib.gs_mesh_decimate_emit):
        assert call(fn, None) == 1
        for kw in (dict(V=0), dict(F=0), dict(V=2 ** 30 + 1), dict(F=(2 ** 31 - 1) // 3 + 1), dict(verts=None), dict(faces=None), dict(counts=None), dict(ws=None),
                   dict(ws=260), dict(cell_size=0.0), dict(cell_size=-1.0), dict(cell_size=float("nan")),
                   dict(cell_size=float("inf"))):
            assert call(fn, desc(**kw)) == 1, kw
        assert call(fn, desc(ws_bytes=need - 1)) == 3
    for kw in (dict(V_out=-1), dict(F_out=-1), dict(V_out=V + 1), dict(F_out=F + 1), dict(verts_out=None), dict(faces_out=None),
               dict(colors_out=256)):
        assert call(lib.gs_mesh_decimate_emit, desc(**kw)) == 1, kw


# ---- the export tool ----------------------------------------------------------------------------------------------------------
def test_export_tool_bytes(gs, sphere, tmp_path):
    """without the new flags the tool's decimation step returns the very tensors it was given and the file is byte-identical;
    with them the file holds gs.mesh_decimate's mesh.  (The tool's full run over a generated dataset needs a GPU:
    tests/test_gpu_meshdecimate.py::test_export_tool_on_the_generated_dataset runs it with and without the flags.)"""
    spec = importlib.util.spec_from_file_location("export_mesh_tool_decimate", ROOT / "tools" / "export_mesh.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    verts, faces, colors = (torch.from_numpy(a) for a in sphere)
    v, f, c, extra = tool.decimate_mesh(verts, faces, colors, 1.0)
    assert v is verts and f is faces and c is colors and extra == {}
    gs.tsdf.write_mesh_ply(tmp_path / "plain.ply", verts, faces, colors)
    gs.tsdf.write_mesh_ply(tmp_path / "default.ply", v, f, c)
    assert (tmp_path / "default.ply").read_bytes() == (tmp_path / "plain.ply").read_bytes()
    v, f, c, extra = tool.decimate_mesh(verts, faces, colors, 1.0, decimate_cell=2.0)
    want = gs.mesh_decimate(verts, faces, colors, cell_size=2.0)
    assert all(torch.equal(a, b) for a, b in zip((v, f, c), want)) and extra["decimate_cell"] == 2.0
    assert extra["faces_before_decimation"] == len(faces) and len(f) < len(faces)
    v, f, c, extra = tool.decimate_mesh(verts, faces, colors, 1.0, target_faces=1000)
    want = gs.mesh_decimate(verts, faces, colors, cell_size=1.0, target_faces=1000)
    assert all(torch.equal(a, b) for a, b in zip((v, f, c), want)) and len(f) <= 1000 and extra["decimate_cell"] > 1.0
    gs.tsdf.write_mesh_ply(tmp_path / "small.ply", v, f, c)
    v2, f2, _ = gs.tsdf.read_mesh_ply(tmp_path / "small.ply")
    assert torch.equal(v2, v) and torch.equal(f2, f)
    assert (tmp_path / "small.ply").stat().st_size < (tmp_path / "plain.ply").stat().st_size // 4
    src = (ROOT / "tools" / "export_mesh.py").read_text()
    assert src.index("clean_mesh(verts") < src.index("decimate_mesh(verts, faces, colors, volume.voxel_size")     # clean, then decimate
    with pytest.raises(ValueError, match="cell_size"):           # a cell of 0 is refused, not replaced by the voxel size
        tool.decimate_mesh(verts, faces, colors, 1.0, decimate_cell=0.0)


# ---- sanitizers ---------------------------------------------------------------------------------------------------------------
def test_host_build_under_sanitizers(tmp_path):
    """meshdecimate_host.cpp as a program of its own (its main runs the small cases) under the address and
    undefined-behaviour sanitizers"""
    exe = tmp_path / "meshdecimate_host_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-DMESHDECIMATE_HOST_MAIN", f"-I{HDR.parent}", str(SRC), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "ERROR" not in out.stderr and "runtime error" not in out.stderr
