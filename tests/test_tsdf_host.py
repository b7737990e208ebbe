"""TSDF fusion and mesh extraction on the CPU: csrc/tsdf_math.h compiled with g++ (tests/host_math/tsdf_host.cpp visits the
voxels and samples one after the other) and the torch restatements of tsdf.py, both against the float64 reference of
tests/tsdf_reference.py on the cases of tests/test_gpu_tsdf.py; the mesh PLY; SplatfactoDeblurModel.fuse_tsdf; the C-ABI
entries; the host build under the address and undefined-behaviour sanitizers as a program of its own.

Tolerances: tsdf and colour atol = 1e-5 (averages of values in [-1, 1] and [0, 1] over <= 17 float32 updates), weight
exact, outside the fragile voxels (tsdf_reference's docstring; at most 3 % of a case); vertices rtol = 1e-6, faces exact."""
import ctypes
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import tsdf_reference as R

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "host_math" / "tsdf_host.cpp"
LIB = ROOT / "tests" / "host_math" / "libtsdf_host.so"
HDR = ROOT / "3dgs-deblur_amd" / "csrc" / "tsdf_math.h"
HIP = ROOT / "3dgs-deblur_amd" / "csrc" / "tsdf.hip"
K = int(re.search(r"constexpr int kFramesPerLaunch = (\d+);", HDR.read_text()).group(1))
COUNT_BLOCK = int(re.search(r"constexpr int kCountBlock = (\d+);", HIP.read_text()).group(1))
NEW_EXPORTS = {"gs_tsdf_integrate": 23, "gs_tsdf_mesh_workspace_bytes": 3, "gs_tsdf_mesh_count": 11, "gs_tsdf_mesh_emit": 18}
_P, _I, _F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float


def P(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def th():
    if not LIB.exists() or LIB.stat().st_mtime < max(SRC.stat().st_mtime, HDR.stat().st_mtime):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", f"-I{HDR.parent}",
                               str(SRC), "-o", str(LIB)])
    lib = ctypes.CDLL(str(LIB))
    lib.tsh_integrate.argtypes = [_I, _I, _I, _F, _F, _F, _F, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _F, _F, _F, _F]
    lib.tsh_mesh.argtypes = [_I, _I, _I, _F, _F, _F, _F, _P, _P, _P, _F, _F, _P, _P, _P, _P]
    lib.tsh_case_triangle.argtypes = [_I, _I, _I, _P, _P]
    return lib


def host_integrate(th, origin, voxel_size, dims, depth, views, intr, trunc, color=None, weights=None, depth_min=0.0,
                   depth_max=math.inf, max_weight=64.0):
    nx, ny, nz = dims
    f, w = np.ones((nz, ny, nx), np.float32), np.zeros((nz, ny, nx), np.float32)
    c = None if color is None else np.zeros((nz, ny, nx, 3), np.float32)
    arrs = [np.ascontiguousarray(a) if a is not None else None for a in (depth, views, intr, color, weights)]
    assert th.tsh_integrate(nx, ny, nz, *origin, voxel_size, P(f), P(w), P(c), len(depth), depth.shape[1], depth.shape[2],
                            *(P(a) for a in arrs), trunc, depth_min, depth_max, max_weight) == 0
    return f, w, c


def host_mesh(th, origin, voxel_size, tsdf, weight, color=None, level=0.0, min_weight=0.0):
    nz, ny, nx = tsdf.shape
    tsdf, weight = np.ascontiguousarray(tsdf, np.float32), np.ascontiguousarray(weight, np.float32)
    color = None if color is None else np.ascontiguousarray(color, np.float32)
    counts = np.zeros(2, np.int32)
    args = (nx, ny, nz, *origin, voxel_size, P(tsdf), P(weight), P(color), level, min_weight, P(counts))
    assert th.tsh_mesh(*args, None, None, None) == 0
    V, F = int(counts[0]), int(counts[1])
    verts, faces = np.zeros((V, 3), np.float32), np.zeros((F, 3), np.int32)
    cols = None if color is None else np.zeros((V, 3), np.float32)
    if V or F:
        assert th.tsh_mesh(*args, P(verts), P(faces), P(cols)) == 0
    return verts, faces, cols


def volume_of(gs, origin, voxel_size, tsdf, weight, color=None, device="cpu"):
    nz, ny, nx = tsdf.shape
    vol = gs.TSDFVolume(origin, voxel_size, (nx, ny, nz), device=device, color=color is not None)
    vol.tsdf.copy_(torch.from_numpy(np.ascontiguousarray(tsdf, np.float32)))
    vol.weight.copy_(torch.from_numpy(np.ascontiguousarray(weight, np.float32)))
    if color is not None:
        vol.color.copy_(torch.from_numpy(np.ascontiguousarray(color, np.float32)))
    return vol


def torch_integrate(gs, device, frames, trunc, color=True, **kw):
    """frames: numpy (depth, color, views, intr[, weights]) -> the volume's arrays"""
    vol = gs.TSDFVolume(R.SMALL["origin"], R.SMALL["voxel_size"], R.SMALL["dims"], device=device, color=color)
    depth, col, views, intr = (torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in frames[:4])
    weights = torch.from_numpy(frames[4]).to(device) if len(frames) > 4 else None
    gs.tsdf_integrate(vol, depth, views, intr, trunc, color=col if color else None, weights=weights, **kw)
    return vol


def arrays(vol):
    return (vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy(), None if vol.color is None else vol.color.cpu().numpy())


def torch_mesh(gs, vol, **kw):
    v, f, c = gs.tsdf_extract_mesh(vol, **kw)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.device == vol.device
    return v.cpu().numpy(), f.cpu().numpy(), None if c is None else c.cpu().numpy()


# ---- pieces of the header -----------------------------------------------------------------------------------------------
def test_header_tables_against_the_rules(th, gs):
    assert th.tsh_frames_per_launch() == K == gs.tsdf.FRAMES_PER_LAUNCH
    for tet, order in enumerate(R.AXIS_ORDERS):
        at, corners = [0, 0, 0], [0]
        for axis in order:
            at[axis] = 1
            corners.append(at[0] | at[1] << 1 | at[2] << 2)
        assert [th.tsh_tet_corner(tet, n) for n in range(4)] == corners == [gs.tsdf._tet_corner(tet, n) for n in range(4)]
        parity = round(np.linalg.det(np.eye(3)[list(order)]))
        assert th.tsh_tet_odd(tet) == (parity < 0) == gs.tsdf.TET_ODD[tet]
    for t, d in enumerate(R.EDGE_TYPES):
        code = d[0] | d[1] << 1 | d[2] << 2
        assert th.tsh_edge_code_of_type(t) == code == gs.tsdf.EDGE_CODES[t] and th.tsh_edge_type_of_code(code) == t
    for m in range(16):
        for odd in (0, 1):
            want = gs.tsdf._case_triangles(m, odd)
            assert th.tsh_case_triangles(m) == len(want)
            for tri, t in enumerate(want):
                ea, eb = np.zeros(3, np.int32), np.zeros(3, np.int32)
                th.tsh_case_triangle(m, odd, tri, P(ea), P(eb))
                assert list(zip(ea.tolist(), eb.tolist())) == t


# ---- integrate ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", R.small_counts(K))
def test_integrate_ring(th, gs, B):
    scene, refs = R.cached_small(K)
    frames = tuple(a[:B] for a in scene)
    got = host_integrate(th, R.SMALL["origin"], R.SMALL["voxel_size"], R.SMALL["dims"], frames[0], frames[2], frames[3],
                         R.SMALL_TRUNC, color=frames[1])
    R.check_volume(got, refs[B], f"host B={B}")
    tv = arrays(torch_integrate(gs, "cpu", frames, R.SMALL_TRUNC))
    R.check_volume(tv, refs[B], f"torch B={B}")
    assert all(np.array_equal(a, b) for a, b in zip(got, tv))          # the two restatements: the same bits


def test_integrate_hard_case(th, gs):
    depth, color, weights, views, intr, depth_max = R.hard_scene()
    ref = R.cached_hard()
    zz, yy, xx = np.meshgrid(*(o + R.SMALL["voxel_size"] * np.arange(n) for o, n in
                               zip(R.SMALL["origin"][::-1], R.SMALL["dims"][::-1])), indexing="ij")
    z1 = views[1, 2, 0] * xx + views[1, 2, 1] * yy + views[1, 2, 2] * zz + views[1, 2, 3]
    assert (z1 < 0).mean() > 0.1 and (z1 > 0).mean() > 0.1                     # camera 1 sits inside the volume
    kw = dict(depth_min=0.5, depth_max=depth_max)
    got = host_integrate(th, R.SMALL["origin"], R.SMALL["voxel_size"], R.SMALL["dims"], depth, views, intr, R.SMALL_TRUNC,
                         color=color, weights=weights, **kw)
    R.check_volume(got, ref, "host hard")
    tv = arrays(torch_integrate(gs, "cpu", (depth, color, views, intr, weights), R.SMALL_TRUNC, **kw))
    R.check_volume(tv, ref, "torch hard")
    assert all(np.array_equal(a, b) for a, b in zip(got, tv))
    assert ((ref[1] > 0) & (ref[1] != np.round(ref[1]))).any()                 # the half weights arrived
    assert (ref[1] == 0).any()                                                 # and some voxels nobody saw


def test_integrate_chunking_and_repeat(gs):
    scene, _ = R.cached_small(K)
    one = torch_integrate(gs, "cpu", scene, R.SMALL_TRUNC)
    again = torch_integrate(gs, "cpu", scene, R.SMALL_TRUNC)
    single = gs.TSDFVolume(R.SMALL["origin"], R.SMALL["voxel_size"], R.SMALL["dims"])
    uneven = gs.TSDFVolume(R.SMALL["origin"], R.SMALL["voxel_size"], R.SMALL["dims"])
    d, c, v, i = (torch.from_numpy(a) for a in scene)
    for b in range(K + 1):
        gs.tsdf_integrate(single, d[b:b + 1], v[b:b + 1], i[b:b + 1], R.SMALL_TRUNC, color=c[b:b + 1])
    for s in (slice(0, 5), slice(5, K + 1)):
        gs.tsdf_integrate(uneven, d[s], v[s], i[s], R.SMALL_TRUNC, color=c[s])
    for other in (again, single, uneven):
        assert torch.equal(one.tsdf, other.tsdf) and torch.equal(one.weight, other.weight) and torch.equal(one.color, other.color)


def weight_cap_case():
    """5 frames of the ring scene into a 4 x 3 x 2 corner of the small volume -> (kwargs of the volume, frames, capped
    reference, uncapped reference)"""
    scene, _ = R.cached_small(K)
    frames = tuple(a[:5] for a in scene)
    geo = dict(origin=(0.05, 0.02, -0.11), voxel_size=0.0625, dims=(4, 3, 2))       # placed so that no voxel is fragile
    ref = [R.integrate(geo["origin"], geo["voxel_size"], geo["dims"], frames[0], frames[2], frames[3], R.SMALL_TRUNC,
                       color=frames[1], max_weight=mw) for mw in (2.0, 64.0)]
    return geo, frames, ref[0], ref[1]


def test_weight_cap(th, gs):
    geo, frames, capped, free = weight_cap_case()
    assert (free[1] >= 4).all() and (free[1] == 5).any() and (capped[1] == 2).all()    # 4 or 5 of the 5 frames reach a voxel
    assert np.abs(capped[0] - free[0]).max() > 1e-3                            # the cap changes the value
    got = host_integrate(th, geo["origin"], geo["voxel_size"], geo["dims"], frames[0], frames[2], frames[3], R.SMALL_TRUNC,
                         color=frames[1], max_weight=2.0)
    assert (got[1] == 2).all()
    R.check_volume(got, capped, "host cap")
    vol = gs.TSDFVolume(**geo)
    d, c, v, i = (torch.from_numpy(np.ascontiguousarray(a)) for a in frames)
    gs.tsdf_integrate(vol, d, v, i, R.SMALL_TRUNC, color=c, max_weight=2.0)
    R.check_volume(arrays(vol), capped, "torch cap")


def test_size_limits_and_bad_arguments(th, gs):
    assert th.tsh_dims_ok(1024, 1024, 1024) == 1 and th.tsh_dims_ok(1024, 1024, 1025) == 0
    assert th.tsh_dims_ok(1, 8, 8) == 0 and th.tsh_dims_ok(2, 2, 2) == 1
    for dims in ((1024, 1024, 1025), (1, 8, 8), (8, 8, 1), (8, 8)):
        with pytest.raises(ValueError):
            gs.TSDFVolume((0, 0, 0), 0.1, dims)
    with pytest.raises(ValueError):
        gs.TSDFVolume((0, 0, 0), 0.0, (4, 4, 4))
    vol = gs.TSDFVolume((0, 0, 0), 0.1, (4, 4, 4))
    z = torch.zeros
    with pytest.raises(ValueError):
        gs.tsdf_integrate(vol, z(1, 4, 4), z(1, 3, 4), z(1, 4), 0.1, color=z(1, 4, 4, 3))       # viewmats
    with pytest.raises(ValueError):
        gs.tsdf_integrate(vol, z(1, 4, 4), z(1, 4, 4, 4), z(1, 4), 0.1)                         # colour missing
    with pytest.raises(ValueError):
        gs.tsdf_integrate(vol, z(1, 4, 4), z(1, 4, 4, 4), z(1, 4), 0.0, color=z(1, 4, 4, 3))    # trunc
    with pytest.raises(ValueError, match="no CPU fallback"):
        gs.tsdf.tsdf_integrate_hip(vol, z(1, 4, 4), z(1, 4, 4, 4), z(1, 4), 0.1, color=z(1, 4, 4, 3))


def test_c_abi_refuses_before_any_launch(gs):
    """null pointers and sizes outside the limits return 1 on the host: nothing is launched (there is no GPU here)"""
    lib = gs._lib.load()
    for name, n in NEW_EXPORTS.items():
        sig = gs._lib._SIGS.get(name) or gs._lib._SIGS_LL[name]
        assert len(sig) == n, name
    inf = float("inf")
    assert lib.gs_tsdf_integrate(8, 8, 8, 0, 0, 0, 0.1, None, None, None, 1, 4, 4, None, None, None, None, None, 0.1, 0.0, inf,
                                 64.0, None) == 1
    fake = ctypes.c_void_p(256)
    assert lib.gs_tsdf_integrate(1024, 1024, 1025, 0, 0, 0, 0.1, fake, fake, None, 1, 4, 4, fake, fake, fake, None, None, 0.1,
                                 0.0, inf, 64.0, None) == 1
    assert lib.gs_tsdf_integrate(8, 8, 1, 0, 0, 0, 0.1, fake, fake, None, 1, 4, 4, fake, fake, fake, None, None, 0.1, 0.0, inf,
                                 64.0, None) == 1
    assert lib.gs_tsdf_integrate(8, 8, 8, 0, 0, 0, 0.1, fake, fake, None, 1, 4, 4, fake, fake, fake, None, None, 0.0, 0.0, inf,
                                 64.0, None) == 1                                   # trunc
    assert lib.gs_tsdf_integrate(8, 8, 8, 0, 0, 0, 0.1, fake, fake, fake, 1, 4, 4, fake, fake, fake, None, None, 0.1, 0.0, inf,
                                 64.0, None) == 1                                   # colour volume without colour images
    assert lib.gs_tsdf_mesh_workspace_bytes(1024, 1024, 1025) == -1 and lib.gs_tsdf_mesh_workspace_bytes(1, 2, 2) == -1
    n = 64 * 64 * 64
    assert 6 * n < lib.gs_tsdf_mesh_workspace_bytes(64, 64, 64) < 7 * n
    assert lib.gs_tsdf_mesh_count(8, 8, 8, None, None, 0.0, 0.0, None, None, 0, None) == 1
    assert lib.gs_tsdf_mesh_count(8, 8, 8, fake, fake, 0.0, 0.0, fake, fake, 16, None) == 3      # workspace too small
    assert lib.gs_tsdf_mesh_emit(8, 8, 8, 0, 0, 0, 0.1, None, None, 0.0, 1, 1, None, None, None, None, 0, None) == 1
    assert lib.gs_tsdf_mesh_emit(8, 8, 8, 0, 0, 0, 0.1, fake, None, 0.0, -1, 1, fake, fake, None, fake, 1 << 20, None) == 1


# ---- extraction -----------------------------------------------------------------------------------------------------------
def both_meshes(th, gs, origin, voxel_size, f, w, col, what, ref=None, **kw):
    ref = R.extract(origin, voxel_size, f, w, col, **kw) if ref is None else ref
    hm = host_mesh(th, origin, voxel_size, f, w, col, **kw)
    R.check_mesh(hm, ref, f"host {what}")
    tm = torch_mesh(gs, volume_of(gs, origin, voxel_size, f, w, col), **kw)
    R.check_mesh(tm, ref, f"torch {what}")
    assert np.array_equal(hm[0], tm[0]) and np.array_equal(hm[1], tm[1])       # the same float32 operations
    return ref


def test_single_inside_sample(th, gs):
    f = np.ones((5, 5, 5), np.float32)
    f[2, 2, 2] = -1.0
    verts, faces, _, _ = both_meshes(th, gs, R.MESH_ORIGIN, 1.0, f, np.ones_like(f), None, "single sample")
    assert len(verts) == 14 and len(faces) == 24
    assert R.is_closed(faces) and R.euler(verts, faces) == 2
    assert abs(R.signed_volume(verts, faces) - 0.5) < 1e-12


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_sphere_and_torus(th, gs, name):
    f, w, col, ref = R.cached_extract(name)
    verts, faces = ref[0], ref[1]
    both_meshes(th, gs, R.MESH_ORIGIN, 1.0, f, w, col, name, ref=ref)
    assert R.is_closed(faces)
    assert R.face_areas(verts, faces).min() > 0
    vol = R.signed_volume(verts, faces)
    if name == "sphere":
        exact, chi, tol = 4.0 / 3.0 * math.pi * R.SPHERE_R ** 3, 2, 0.01
    else:
        exact, chi, tol = 2.0 * math.pi ** 2 * R.TORUS_R * R.TORUS_r ** 2, 0, 0.03
    print(f"{name}: V {len(verts)}, F {len(faces)}, volume {vol:.1f} of {exact:.1f} ({100 * (1 - vol / exact):.2f} % below)")
    assert R.euler(verts, faces) == chi
    assert 0 < vol < exact and vol > (1 - tol) * exact


def unobserved_case():
    """a tilted plane through a 12 x 10 x 9 volume whose far half (i >= 6) has weight 0"""
    x, y, z = R.grid_points((12, 10, 9))
    f = np.clip((z - (3.0 + 4.2 + 0.21 * (x - 1.0) - 0.13 * (y - 2.0))) / 3.0, -1, 1).astype(np.float32)
    w = np.ones_like(f)
    w[:, :, 6:] = 0.0
    return f, w


def check_unobserved(mesh, w):
    verts, faces, _, cells = mesh
    single, bad = R.boundary_edges(faces)
    assert len(faces) > 0 and single > 0 and bad == 0                          # open, and nowhere more than two faces
    assert set(np.unique(faces).tolist()) == set(range(len(verts)))            # no vertex unreferenced
    nz, ny, nx = w.shape
    for cell in np.unique(cells).tolist():
        i, j, k = cell % nx, (cell // nx) % ny, cell // (nx * ny)
        assert (w[k:k + 2, j:j + 2, i:i + 2] > 0).all()
    assert verts[:, 0].max() <= R.MESH_ORIGIN[0] + 5.0                          # nothing beyond the last observed sample


def test_unobserved_samples(th, gs):
    f, w = unobserved_case()
    ref = both_meshes(th, gs, R.MESH_ORIGIN, 1.0, f, w, None, "unobserved")
    check_unobserved(ref, w)
    # a weight threshold does the same as weight 0
    ref2 = both_meshes(th, gs, R.MESH_ORIGIN, 1.0, f, np.where(w > 0, 3.0, 1.5).astype(np.float32), None, "min_weight",
                       min_weight=2.0)
    assert np.array_equal(ref2[1], ref[1])


@pytest.mark.parametrize("case", ["outside", "inside", "unseen"])
def test_empty_results(th, gs, case):
    f = np.full((4, 5, 6), -1.0 if case == "inside" else 1.0, np.float32)
    if case == "unseen":
        f[1:3, 1:3, 1:3] = -1.0
    w = np.zeros_like(f) if case == "unseen" else np.ones_like(f)
    for col in (None, np.zeros(f.shape + (3,), np.float32)):
        hm = host_mesh(th, R.MESH_ORIGIN, 1.0, f, w, col)
        v, fc, c = gs.tsdf_extract_mesh(volume_of(gs, R.MESH_ORIGIN, 1.0, f, w, col))
        assert hm[0].shape == (0, 3) and hm[1].shape == (0, 3)
        assert tuple(v.shape) == (0, 3) and tuple(fc.shape) == (0, 3) and v.dtype == torch.float32 and fc.dtype == torch.int32
        assert (c is None) == (col is None) and (c is None or (tuple(c.shape) == (0, 3) and c.dtype == torch.float32))


def block_dims():
    """volumes whose sample counts sit just below, at and above the count kernel's workgroup (the unit the scan works in)"""
    assert COUNT_BLOCK == 256
    return [(5, 7, 7), (8, 8, 4), (3, 9, 10)]


@pytest.mark.parametrize("dims", block_dims())
def test_block_boundaries(th, gs, dims):
    f, w, col, ref = R.cached_extract("blocks", dims)
    assert len(ref[1]) > 0
    both_meshes(th, gs, R.MESH_ORIGIN, 1.0, f, w, col, f"blocks {dims}", ref=ref)


def test_mesh_ply_round_trip(gs, tmp_path):
    f, w, col, ref = R.cached_extract("sphere")
    verts, faces, cols = (torch.from_numpy(a) for a in ref[:3])
    path = tmp_path / "mesh.ply"
    gs.tsdf.write_mesh_ply(path, verts.float(), faces.int(), cols.float())
    head = path.read_bytes()[:400].decode("ascii", "replace")
    assert "format binary_little_endian 1.0" in head and "property list uchar int vertex_indices" in head
    assert "property uchar red" in head
    v2, f2, c2 = gs.tsdf.read_mesh_ply(path)
    assert torch.equal(v2, verts.float()) and torch.equal(f2, faces.int()) and f2.dtype == torch.int32
    assert float((c2 - cols.float()).abs().max()) <= 0.5 / 255 + 1e-6
    gs.tsdf.write_mesh_ply(path, verts.float(), faces.int())                   # overwritten in place, without colours
    v3, f3, c3 = gs.tsdf.read_mesh_ply(path)
    assert c3 is None and torch.equal(f3, faces.int()) and torch.equal(v3, verts.float())
    assert [p.name for p in tmp_path.iterdir()] == ["mesh.ply"]                # no temporary file left
    with pytest.raises(ValueError):
        gs.tsdf.write_mesh_ply(path, verts.float(), faces.int() + len(verts))


# ---- end to end -----------------------------------------------------------------------------------------------------------
E2E_HOST_N = 24
E2E_HOST_MEASURED = 0.06720                # tsdf_reference.integrate_frames + extract on e2e_scene(24), voxel 0.08696


def e2e_error(verts, center, radius):
    return float(np.abs(np.linalg.norm(np.asarray(verts, np.float64) - np.asarray(center), axis=1) - radius).max())


def test_end_to_end_sphere_host(gs):
    """depth maps of a sphere ray-cast in numpy, fused and meshed by the torch restatements at 24^3: the mesh is closed and
    max | |v - c| - r | stays within 1.5 x what the float64 reference gives on the same scene (measured: 0.06720,
    0.77 voxel; the test checks that figure too)."""
    origin, vs, dims, depth, views, intr, trunc, center, radius = R.e2e_scene(E2E_HOST_N)
    vol = gs.TSDFVolume(origin, vs, dims, color=False)
    gs.tsdf_integrate(vol, torch.from_numpy(depth), torch.from_numpy(views), torch.from_numpy(intr), trunc)
    verts, faces, _ = gs.tsdf_extract_mesh(vol)
    err = e2e_error(verts.numpy(), center, radius)
    print(f"end to end {E2E_HOST_N}^3: V {len(verts)}, F {len(faces)}, max radial error {err:.5f} (voxel {vs:.5f})")
    assert R.is_closed(faces.numpy()) and R.euler(verts.numpy(), faces.numpy()) == 2
    assert err <= 1.5 * E2E_HOST_MEASURED
    t, w = R.integrate_frames(origin, vs, dims, depth, views, intr, trunc)
    ref = R.extract(origin, vs, t, w)
    assert abs(e2e_error(ref[0], center, radius) - E2E_HOST_MEASURED) < 1e-5


# ---- sanitizers -----------------------------------------------------------------------------------------------------------
def test_host_build_under_sanitizers(tmp_path):
    """tsdf_host.cpp as a program of its own (its main runs the small cases) under the address and undefined-behaviour
    sanitizers"""
    exe = tmp_path / "tsdf_host_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-DTSDF_HOST_MAIN", f"-I{HDR.parent}", str(SRC), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "ERROR" not in out.stderr and "runtime error" not in out.stderr


# ---- model ----------------------------------------------------------------------------------------------------------------
def gl_camera(gs, eye, target, W, H, f, **metadata):
    """a gs.Camera (OpenGL camera_to_world) looking from eye at target"""
    m = R.look_at(eye, target)
    c2w = np.zeros((3, 4))
    c2w[:, :3] = m[:3, :3].T * np.array([1.0, -1.0, -1.0])[None, :]
    c2w[:, 3] = eye
    return gs.Camera(torch.tensor(c2w, dtype=torch.float32), f, f, W / 2, H / 2, W, H, dict(metadata))


def tiny_model(gs, shutter=False, n=400):
    cfg = gs.SplatfactoDeblurConfig(sh_degree=1, blur_samples=5)
    cfg.camera_optimizer.mode = "SO3xR3"
    if shutter:
        cfg.camera_shutter_optimizer.exposure = "global"
        cfg.camera_shutter_optimizer.initial_exposure_time = 0.02
    g = torch.Generator().manual_seed(2)
    means = (torch.rand(n, 3, generator=g) - 0.5) * 1.6
    return gs.SplatfactoDeblurModel(cfg, means, torch.full((n, 3), math.log(0.01)), torch.ones(n, 4), torch.zeros(n),
                                    torch.zeros(n, 3), torch.zeros(n, 3, 3), 8)


def sphere_render(model, calls):
    """a CPU stand-in for the HIP render: the z-depth of a sphere of radius 0.5 at the origin from the model's own
    viewmat, accumulation 1 where the ray hits; records what the model scheduled for the camera"""
    def render(camera, detach_gaussians=False, return_depth=None):
        S, Rb, times = model._schedule(camera)
        calls.append(dict(S=S, R=Rb, times=list(times), cam_idx=camera.metadata.get("cam_idx"), training=model.training,
                          exposure=float(model.shutter_times(camera)[0]), size=(camera.height, camera.width)))
        view = model._viewmat_and_velocity(camera)[0].detach().numpy()[None]
        intr = np.float32([[camera.fx, camera.fy, camera.cx, camera.cy]])
        depth = R.raycast_sphere_depth(view, intr, camera.height, camera.width, (0.0, 0.0, 0.0), 0.5, far=0.0)[0]
        hit = torch.from_numpy(depth > 0).float()
        return {"rgb": hit[..., None] * torch.tensor([0.2, 0.6, 0.9]), "depth": torch.from_numpy(depth)[..., None],
                "accumulation": hit[..., None], "background": None}
    return render


def model_cameras(gs):
    cams = []
    for n, (W, H) in enumerate([(48, 32), (48, 32), (48, 32), (40, 30), (40, 30), (48, 32)]):
        a = 0.3 + n
        cams.append(gl_camera(gs, (2.2 * math.cos(a), 2.2 * math.sin(a), 0.5), (0, 0, 0), W, H, 45.0, cam_idx=n,
                              exposure_time=0.01, rolling_shutter_time=0.02, camera_linear_velocity=(0.3, 0.0, 0.1),
                              camera_angular_velocity=(0.0, 0.2, 0.0)))
    return cams


@pytest.mark.parametrize("shutter", [False, True])
def test_fuse_tsdf_on_cpu_tensors(gs, monkeypatch, shutter):
    model = tiny_model(gs, shutter)
    calls, batches = [], []
    monkeypatch.setattr(model, "_render", sphere_render(model, calls))
    real = gs.tsdf.tsdf_integrate
    monkeypatch.setattr(gs.tsdf, "tsdf_integrate", lambda vol, depth, *a, **k: (batches.append(tuple(depth.shape)), real(vol, depth, *a, **k))[1])
    cams = model_cameras(gs)
    model.train()
    vol = model.fuse_tsdf(cams, resolution=24, batch=2)
    assert model.training and not model._sharp                                  # both restored
    assert isinstance(vol, gs.TSDFVolume) and max(vol.dims) == 24 and vol.color is not None
    assert float(vol.weight.sum()) > 0 and float(vol.tsdf.min()) < 0 < float(vol.tsdf.max())
    # sharp: one sample at time 0 for every camera, in eval mode, cam_idx kept, the learned exposure counted as 0
    assert [c["cam_idx"] for c in calls] == list(range(6))
    assert all(c["S"] == 1 and c["R"] == 1 and c["times"] == [0.0] and c["exposure"] == 0.0 and not c["training"] for c in calls)
    assert batches == [(2, 32, 48), (1, 32, 48), (2, 30, 40), (1, 32, 48)]      # cameras of another size start a new call
    assert model._schedule(cams[0])[0] == 5                                     # outside, the camera blurs as before
    verts, faces, colors = gs.tsdf_extract_mesh(vol)
    assert len(faces) > 0 and float((verts.norm(dim=1) - 0.5).abs().max()) < 2.5 * vol.voxel_size
    assert torch.allclose(colors.mean(dim=0), torch.tensor([0.2, 0.6, 0.9]), atol=0.05)
    # blurred on request, into a volume of the caller's, with the default batch
    calls.clear(), batches.clear()
    own = gs.TSDFVolume((-0.8, -0.8, -0.8), 0.1, (17, 17, 17))
    assert model.fuse_tsdf(cams[:3], volume=own, sharp=False) is own
    assert all(c["S"] == 5 for c in calls) and batches == [(3, 32, 48)] and float(own.weight.sum()) > 0


def test_fuse_tsdf_bounds_and_errors(gs, monkeypatch):
    model = tiny_model(gs)
    monkeypatch.setattr(model, "_render", sphere_render(model, []))
    cams = model_cameras(gs)[:2]
    vol = model.fuse_tsdf(cams, resolution=16, bounds=((-1.0, -0.5, -0.25), (1.0, 0.5, 0.25)))
    assert vol.dims == (16, 9, 5) and vol.origin == (-1.0, -0.5, -0.25) and vol.voxel_size == pytest.approx(2.0 / 15)
    lo = model.means.detach().sort(dim=0).values[int(0.02 * 399)]
    auto = model.fuse_tsdf(cams, resolution=16)
    assert all(o < float(v) for o, v in zip(auto.origin, lo)) and max(auto.dims) == 16
    with pytest.raises(ValueError):
        model.fuse_tsdf(cams, resolution=1)

    def failing(camera, *a, **kw):
        raise RuntimeError("render failed")
    monkeypatch.setattr(model, "_render", failing)
    with pytest.raises(RuntimeError):
        model.fuse_tsdf(cams, resolution=16)
    assert not model._sharp
