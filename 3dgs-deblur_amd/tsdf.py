"""TSDF fusion of rendered depth maps into a volume, and a coloured triangle mesh from it (nerfstudio's ``ns-export tsdf``).

The volume: ``tsdf`` and ``weight`` [nz,ny,nx], ``color`` [nz,ny,nx,3] float32, x fastest; sample (i, j, k) sits at
``origin + voxel_size * (i, j, k)``.  csrc/tsdf_math.h states every operation; in short, for every voxel, frames applied
in index order, float32 with every operation rounded:

  project  p = R x + t, z = p.z, skip the frame if z <= 0; u = fx p.x / z + cx, v = fy p.y / z + cy;
           px = floor(u), py = floor(v) (pixel centres at +0.5, as in the rasterizer); skip outside the image
  depth    D = depth[b, py, px], w = weights[b, py, px] (1 without weights); skip unless D is finite,
           depth_min < D <= depth_max and w > 0; sdf = D - z; skip if sdf < -trunc; val = min(1, sdf / trunc)
  update   Wn = W + w; tsdf = (tsdf W + val w) / Wn; colour with the same weights; W = min(Wn, max_weight)

``viewmats`` are the renderer's world-to-camera matrices (OpenCV axes, +z forward), ``depth`` is camera-space z (what
``outputs["depth"]`` holds), not ray length.

The mesh is marching tetrahedra on the Kuhn split of every cell (six tetrahedra along the monotone corner paths
000 -> 111, one per order of the axes): every face diagonal runs from a cell's lower to its upper corner, neighbouring
cells agree, the surface is watertight by construction and needs no 256-case table.  A corner is inside when
``tsdf < level``, a cell is used when its 8 corners have ``weight > min_weight``.  Vertices are shared through indices and
ordered by (owner sample, edge type), faces by (cell, tetrahedron, triangle): the result is the same bits every run.

On HIP tensors the kernels of csrc/tsdf.hip are the only route (``gs_tsdf_integrate``: one launch per 16 frames, the
voxel's state in registers across them; ``gs_tsdf_mesh_count`` / ``gs_tsdf_mesh_emit``: count, integer scan, emit, one
8-byte read-back for V and F).  CPU tensors take ``tsdf_integrate_torch`` and ``tsdf_extract_mesh_torch``."""
from __future__ import annotations

import ctypes
import math
import os
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

FRAMES_PER_LAUNCH = 16               # csrc/tsdf_math.h kFramesPerLaunch
MIN_DIM, MAX_DIM = 2, 1024           # kMinDim, kMaxDim
MAX_VOXELS = 1 << 30                 # kMaxVoxels
MAX_IMAGE_DIM = 16384                # kMaxImageDim
# the six tetrahedra: orders of the axes, lexicographic; odd orders are mirrored
TET_AXES = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
TET_ODD = (0, 1, 1, 0, 0, 1)
EDGE_CODES = (1, 2, 4, 3, 5, 6, 7)   # +x +y +z +xy +xz +yz +xyz as corner codes (bit 0 = x)
FLIP_EVEN = 0x4D24                   # kFlipEven


class TSDFVolume:
    """A truncated signed distance volume: tsdf [nz,ny,nx] (1), weight [nz,ny,nx] (0), color [nz,ny,nx,3] (0) or None.
    origin: the position of sample (0, 0, 0); dims = (nx, ny, nz), each 2..1024, nx ny nz <= 2^30."""

    def __init__(self, origin: Sequence[float], voxel_size: float, dims: Sequence[int], device="cpu", color: bool = True):
        origin = tuple(float(o) for o in origin)
        if len(origin) != 3 or not all(math.isfinite(o) for o in origin):
            raise ValueError(f"origin must be three finite numbers, got {origin}")
        voxel_size = float(voxel_size)
        if not (math.isfinite(voxel_size) and voxel_size > 0):
            raise ValueError(f"voxel_size must be positive, got {voxel_size}")
        dims = tuple(int(d) for d in dims)
        if len(dims) != 3 or any(d < MIN_DIM or d > MAX_DIM for d in dims):
            raise ValueError(f"dims must be three sizes between {MIN_DIM} and {MAX_DIM}, got {dims}")
        if dims[0] * dims[1] * dims[2] > MAX_VOXELS:
            raise ValueError(f"a volume holds at most 2^30 samples, got {dims}")
        self.origin, self.voxel_size, self.dims = origin, voxel_size, dims
        nx, ny, nz = dims
        self.tsdf = torch.ones(nz, ny, nx, dtype=torch.float32, device=device)
        self.weight = torch.zeros(nz, ny, nx, dtype=torch.float32, device=device)
        self.color = torch.zeros(nz, ny, nx, 3, dtype=torch.float32, device=device) if color else None

    @property
    def device(self):
        return self.tsdf.device


def _check_frames(volume, depth, viewmats, intrins, trunc, color, weights, max_weight):
    if not isinstance(volume, TSDFVolume):
        raise ValueError("volume must be a TSDFVolume")
    dev = volume.device
    if not isinstance(depth, Tensor) or depth.dim() != 3:
        raise ValueError("depth must be a [B,H,W] tensor")
    B, H, W = (int(s) for s in depth.shape)
    if H < 1 or W < 1 or H > MAX_IMAGE_DIM or W > MAX_IMAGE_DIM:
        raise ValueError(f"images are 1..{MAX_IMAGE_DIM} pixels a side, got {H} x {W}")
    if tuple(viewmats.shape) != (B, 4, 4) or tuple(intrins.shape) != (B, 4):
        raise ValueError(f"viewmats must be [{B},4,4] and intrins [{B},4], got {tuple(viewmats.shape)}, {tuple(intrins.shape)}")
    if (color is None) != (volume.color is None):
        raise ValueError("colour images are given exactly when the volume holds colour")
    if color is not None and tuple(color.shape) != (B, H, W, 3):
        raise ValueError(f"color must be [{B},{H},{W},3], got {tuple(color.shape)}")
    if weights is not None and tuple(weights.shape) != (B, H, W):
        raise ValueError(f"weights must be [{B},{H},{W}], got {tuple(weights.shape)}")
    for name, t in (("depth", depth), ("viewmats", viewmats), ("intrins", intrins), ("color", color), ("weights", weights)):
        if t is None:
            continue
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32")
        if t.device != dev:
            raise ValueError(f"{name} is on {t.device}, the volume on {dev}")
    if not (math.isfinite(float(trunc)) and float(trunc) > 0):
        raise ValueError(f"trunc must be positive, got {trunc}")
    if not float(max_weight) > 0:
        raise ValueError(f"max_weight must be positive, got {max_weight}")
    return B, H, W


def tsdf_integrate_hip(volume: TSDFVolume, depth: Tensor, viewmats: Tensor, intrins: Tensor, trunc: float,
                       color: Optional[Tensor] = None, weights: Optional[Tensor] = None, depth_min: float = 0.0,
                       depth_max: float = math.inf, max_weight: float = 64.0) -> TSDFVolume:
    """gs_tsdf_integrate on GPU tensors (arguments as tsdf_integrate)"""
    from . import _lib
    if not volume.tsdf.is_cuda:
        raise ValueError("the volume must hold CUDA(HIP) tensors: the HIP path has no CPU fallback")
    B, H, W = _check_frames(volume, depth, viewmats, intrins, trunc, color, weights, max_weight)
    if B == 0:
        return volume
    depth, viewmats, intrins = depth.detach().contiguous(), viewmats.detach().contiguous(), intrins.detach().contiguous()
    color = None if color is None else color.detach().contiguous()
    weights = None if weights is None else weights.detach().contiguous()
    lib = _lib.load()
    vp = ctypes.c_void_p

    def ptr(t):
        return vp(None if t is None else t.data_ptr())
    nx, ny, nz = volume.dims
    with torch.cuda.device(volume.device):
        _lib.check(lib.gs_tsdf_integrate(nx, ny, nz, volume.origin[0], volume.origin[1], volume.origin[2],
                                         volume.voxel_size, ptr(volume.tsdf), ptr(volume.weight), ptr(volume.color), B, H, W,
                                         ptr(depth), ptr(viewmats), ptr(intrins), ptr(color), ptr(weights), float(trunc),
                                         float(depth_min), float(depth_max), float(max_weight),
                                         vp(torch.cuda.current_stream().cuda_stream)), "tsdf_integrate")
    return volume


def tsdf_integrate_torch(volume: TSDFVolume, depth: Tensor, viewmats: Tensor, intrins: Tensor, trunc: float,
                         color: Optional[Tensor] = None, weights: Optional[Tensor] = None, depth_min: float = 0.0,
                         depth_max: float = math.inf, max_weight: float = 64.0) -> TSDFVolume:
    """the operations of csrc/tsdf_math.h one by one as torch ops on the volume's device, one frame after the other
    (arguments as tsdf_integrate)"""
    B, H, W = _check_frames(volume, depth, viewmats, intrins, trunc, color, weights, max_weight)
    dev = volume.device
    f32 = dict(dtype=torch.float32, device=dev)
    nx, ny, nz = volume.dims

    def s(v):
        return torch.tensor(float(v), **f32)
    vs = s(volume.voxel_size)
    x = (s(volume.origin[0]) + vs * torch.arange(nx, **f32))[None, None, :]
    y = (s(volume.origin[1]) + vs * torch.arange(ny, **f32))[None, :, None]
    z = (s(volume.origin[2]) + vs * torch.arange(nz, **f32))[:, None, None]
    tr, dmin, dmax, maxw, one = s(trunc), s(depth_min), s(depth_max), s(max_weight), s(1.0)
    Wf, Hf = s(W), s(H)
    f, Wt, col = volume.tsdf, volume.weight, volume.color
    depth, viewmats, intrins = depth.detach(), viewmats.detach(), intrins.detach()
    for b in range(B):
        m, (fx, fy, cx, cy) = viewmats[b], intrins[b]
        pc = [((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3)]
        zc = pc[2]
        ok = zc > 0
        zs = torch.where(ok, zc, one)
        u, v = (fx * pc[0]) / zs + cx, (fy * pc[1]) / zs + cy
        ok = ok & (u >= 0) & (u < Wf) & (v >= 0) & (v < Hf)
        pix = torch.where(ok, torch.floor(v).long() * W + torch.floor(u).long(), torch.zeros((), dtype=torch.long, device=dev))
        D = depth[b].reshape(-1)[pix]
        w = weights[b].detach().reshape(-1)[pix] if weights is not None else torch.ones_like(D)
        ok = ok & torch.isfinite(D) & (D > dmin) & (D <= dmax) & (w > 0)
        sdf = D - zc
        ok = ok & ~(sdf < -tr)
        val = torch.minimum(one, sdf / tr)
        Wn = torch.where(ok, Wt + w, one)
        f = torch.where(ok, (f * Wt + val * w) / Wn, f)
        if col is not None:
            c = color[b].detach().reshape(-1, 3)[pix]
            col = torch.where(ok[..., None], (col * Wt[..., None] + c * w[..., None]) / Wn[..., None], col)
        Wt = torch.where(ok, torch.minimum(Wn, maxw), Wt)
    volume.tsdf.copy_(f)
    volume.weight.copy_(Wt)
    if col is not None:
        volume.color.copy_(col)
    return volume


def tsdf_integrate(volume: TSDFVolume, depth: Tensor, viewmats: Tensor, intrins: Tensor, trunc: float,
                   color: Optional[Tensor] = None, weights: Optional[Tensor] = None, depth_min: float = 0.0,
                   depth_max: float = math.inf, max_weight: float = 64.0) -> TSDFVolume:
    """Fuse B frames into the volume, in place (module docstring: the rule).  depth [B,H,W] camera-space z, viewmats
    [B,4,4] world-to-camera, intrins [B,4] = fx fy cx cy, color [B,H,W,3] (exactly when the volume holds colour), weights
    [B,H,W] or None (1), all float32 on the volume's device.  The result does not depend on how the frames are cut into
    calls.  HIP tensors take the kernel, CPU tensors tsdf_integrate_torch.  Returns the volume."""
    if not isinstance(volume, TSDFVolume):
        raise ValueError("volume must be a TSDFVolume")
    fn = tsdf_integrate_hip if volume.tsdf.is_cuda else tsdf_integrate_torch
    return fn(volume, depth, viewmats, intrins, trunc, color, weights, depth_min, depth_max, max_weight)


# --------------------------------------------------------------------------- #
# mesh extraction
# --------------------------------------------------------------------------- #
def _empty_mesh(dev, color: bool):
    return (torch.zeros(0, 3, dtype=torch.float32, device=dev), torch.zeros(0, 3, dtype=torch.int32, device=dev),
            torch.zeros(0, 3, dtype=torch.float32, device=dev) if color else None)


def tsdf_extract_mesh_hip(volume: TSDFVolume, level: float = 0.0, min_weight: float = 0.0):
    """gs_tsdf_mesh_count, the 8-byte read-back of V and F, gs_tsdf_mesh_emit (result as tsdf_extract_mesh)"""
    from . import _lib
    if not volume.tsdf.is_cuda:
        raise ValueError("the volume must hold CUDA(HIP) tensors: the HIP path has no CPU fallback")
    lib = _lib.load()
    vp = ctypes.c_void_p
    nx, ny, nz = volume.dims
    dev = volume.device
    has_color = volume.color is not None
    with torch.cuda.device(dev):
        ws_bytes = int(lib.gs_tsdf_mesh_workspace_bytes(nx, ny, nz))
        if ws_bytes < 0:
            raise _lib.HipLibraryError(f"tsdf_extract_mesh: unsupported volume {volume.dims}")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        stream = vp(torch.cuda.current_stream().cuda_stream)
        _lib.check(lib.gs_tsdf_mesh_count(nx, ny, nz, vp(volume.tsdf.data_ptr()), vp(volume.weight.data_ptr()), float(level),
                                          float(min_weight), vp(counts.data_ptr()), vp(ws.data_ptr()), ws_bytes, stream),
                   "tsdf_mesh_count")
        V, F = (int(c) for c in counts.tolist())
        if V < 0 or F < 0:
            raise _lib.HipLibraryError("tsdf_extract_mesh: the mesh has more than 2^31 - 1 vertices or faces")
        if V == 0 and F == 0:
            return _empty_mesh(dev, has_color)
        verts = torch.empty(V, 3, dtype=torch.float32, device=dev)
        faces = torch.empty(F, 3, dtype=torch.int32, device=dev)
        colors = torch.empty(V, 3, dtype=torch.float32, device=dev) if has_color else None
        _lib.check(lib.gs_tsdf_mesh_emit(nx, ny, nz, volume.origin[0], volume.origin[1], volume.origin[2], volume.voxel_size,
                                         vp(volume.tsdf.data_ptr()), vp(volume.color.data_ptr() if has_color else None),
                                         float(level), V, F, vp(verts.data_ptr()), vp(faces.data_ptr()),
                                         vp(colors.data_ptr() if has_color else None), vp(ws.data_ptr()), ws_bytes, stream),
                   "tsdf_mesh_emit")
    return verts, faces, colors


def _tet_corner(tet: int, n: int) -> int:
    a, b, _ = TET_AXES[tet]
    return (0, 1 << a, (1 << a) | (1 << b), 7)[n]


def _case_triangles(m: int, odd: int):
    """triangles of the 4-bit case m as lists of three (lower, upper) path-corner pairs, oriented"""
    ins = [n for n in range(4) if (m >> n) & 1]
    out = [n for n in range(4) if not (m >> n) & 1]
    if len(ins) in (0, 4):
        return []
    if len(ins) == 1:
        tris = [[(ins[0], o) for o in out]]
    elif len(ins) == 3:
        tris = [[(out[0], o) for o in ins]]
    else:
        (a, b), (c, d) = ins, out
        tris = [[(a, c), (a, d), (b, d)], [(a, c), (b, d), (b, c)]]
    if ((FLIP_EVEN >> m) & 1) != odd:
        tris = [[t[0], t[2], t[1]] for t in tris]
    return [[(min(p), max(p)) for p in t] for t in tris]


def tsdf_extract_mesh_torch(volume: TSDFVolume, level: float = 0.0, min_weight: float = 0.0):
    """the extraction of csrc/tsdf_math.h on the host: the used cells the surface crosses are found with array ops, then a
    plain loop over them (result as tsdf_extract_mesh, float32 arithmetic as the kernels')"""
    dev = volume.device
    f = volume.tsdf.detach().cpu().numpy()
    w = volume.weight.detach().cpu().numpy()
    col = None if volume.color is None else volume.color.detach().cpu().numpy()
    nx, ny, nz = volume.dims
    lv = np.float32(level)
    inside = f < lv
    seen = w > np.float32(min_weight)

    def corner(a, c):
        dx, dy, dz = c & 1, (c >> 1) & 1, c >> 2
        return a[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
    used = np.ones((nz - 1, ny - 1, nx - 1), bool)
    mask = np.zeros((nz - 1, ny - 1, nx - 1), np.int32)
    for c in range(8):
        used &= corner(seen, c)
        mask |= corner(inside, c).astype(np.int32) << c
    cells = np.argwhere(used & (mask != 0) & (mask != 255))        # (k, j, i) rows in linear order
    tris, edges = [], set()
    for k, j, i in cells.tolist():
        cm = int(mask[k, j, i])
        for tet in range(6):
            m = 0
            for n in range(4):
                m |= ((cm >> _tet_corner(tet, n)) & 1) << n
            for t in _case_triangles(m, TET_ODD[tet]):
                keys = []
                for lo, hi in t:
                    ca, cb = _tet_corner(tet, lo), _tet_corner(tet, hi)
                    owner = ((k + (ca >> 2)) * ny + j + ((ca >> 1) & 1)) * nx + i + (ca & 1)
                    keys.append((owner, EDGE_CODES.index(ca ^ cb)))
                edges.update(keys)
                tris.append(keys)
    if not tris:
        return _empty_mesh(dev, col is not None)
    order = sorted(edges)
    index = {e: n for n, e in enumerate(order)}
    faces = np.array([[index[e] for e in t] for t in tris], np.int32)
    own = np.array([e[0] for e in order], np.int64)
    code = np.array([EDGE_CODES[e[1]] for e in order], np.int64)
    ia, ja, ka = own % nx, (own // nx) % ny, own // (nx * ny)
    ib, jb, kb = ia + (code & 1), ja + ((code >> 1) & 1), ka + (code >> 2)
    fa, fb = f[ka, ja, ia], f[kb, jb, ib]
    t = (lv - fa) / (fb - fa)
    vs = np.float32(volume.voxel_size)
    verts = np.empty((len(order), 3), np.float32)
    for axis, (a, b) in enumerate(((ia, ib), (ja, jb), (ka, kb))):
        o = np.float32(volume.origin[axis])
        pa, pb = o + vs * a.astype(np.float32), o + vs * b.astype(np.float32)
        verts[:, axis] = pa + t * (pb - pa)
    colors = None
    if col is not None:
        ca_, cb_ = col[ka, ja, ia], col[kb, jb, ib]
        colors = torch.from_numpy((ca_ + t[:, None] * (cb_ - ca_)).astype(np.float32)).to(dev)
    return torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev), colors


def tsdf_extract_mesh(volume: TSDFVolume, level: float = 0.0, min_weight: float = 0.0
                      ) -> Tuple[Tensor, Tensor, Optional[Tensor]]:
    """The triangle mesh of the volume's level set (module docstring: the construction) -> (verts [V,3] float32 in world
    units, faces [F,3] int32, colors [V,3] float32 or None) on the volume's device.  Normals point towards increasing
    tsdf, into free space.  Only cells whose 8 corners have weight > min_weight are used; every vertex is referenced.
    HIP tensors take the kernels, CPU tensors tsdf_extract_mesh_torch."""
    if not isinstance(volume, TSDFVolume):
        raise ValueError("volume must be a TSDFVolume")
    if not (math.isfinite(float(level)) and math.isfinite(float(min_weight))):
        raise ValueError("level and min_weight must be finite")
    fn = tsdf_extract_mesh_hip if volume.tsdf.is_cuda else tsdf_extract_mesh_torch
    return fn(volume, level, min_weight)


# --------------------------------------------------------------------------- #
# mesh PLY
# --------------------------------------------------------------------------- #
def write_mesh_ply(path, verts: Tensor, faces: Tensor, colors: Optional[Tensor] = None) -> None:
    """Binary little-endian PLY: vertex x y z float (+ red green blue uchar with colours in [0, 1]), face
    ``list uchar int vertex_indices``.  Written atomically (temporary file beside it, then os.replace)."""
    from .checkpoint import _atomic_write
    v = np.ascontiguousarray(torch.as_tensor(verts).detach().cpu().numpy(), dtype="<f4").reshape(-1, 3)
    fc = np.ascontiguousarray(torch.as_tensor(faces).detach().cpu().numpy(), dtype="<i4").reshape(-1, 3)
    if len(fc) and (fc.min() < 0 or fc.max() >= len(v)):
        raise ValueError("faces refer to vertices that do not exist")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if colors is not None:
        c = torch.as_tensor(colors).detach().cpu().numpy().reshape(-1, 3)
        if len(c) != len(v):
            raise ValueError(f"{len(v)} vertices but {len(c)} colours")
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    vrec = np.zeros(len(v), dtype=fields)
    vrec["x"], vrec["y"], vrec["z"] = v[:, 0], v[:, 1], v[:, 2]
    if colors is not None:
        c8 = np.rint(np.clip(np.nan_to_num(c), 0.0, 1.0) * 255.0).astype(np.uint8)
        vrec["red"], vrec["green"], vrec["blue"] = c8[:, 0], c8[:, 1], c8[:, 2]
    frec = np.zeros(len(fc), dtype=[("n", "u1"), ("v", "<i4", (3,))])
    frec["n"], frec["v"] = 3, fc
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}", "property float x", "property float y",
              "property float z"]
    if colors is not None:
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    header += [f"element face {len(fc)}", "property list uchar int vertex_indices", "end_header"]

    def write(fh):
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())
    _atomic_write(os.fspath(path), write)


def read_mesh_ply(path):
    """-> (verts [V,3] float32, faces [F,3] int32, colors [V,3] float32 in [0, 1] or None), CPU tensors, of a file
    write_mesh_ply wrote (triangles only)"""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    lines = data[:end].decode("ascii").split("\n")
    body = data[end + len(b"end_header\n"):]
    if "format binary_little_endian 1.0" not in lines:
        raise ValueError(f"{path}: only binary little-endian PLY is read")
    elements, current = [], None
    for ln in lines:
        tok = ln.split()
        if tok[:1] == ["element"]:
            current = (tok[1], int(tok[2]), [])
            elements.append(current)
        elif tok[:1] == ["property"] and current is not None:
            current[2].append(tok[1:])
    if [e[0] for e in elements] != ["vertex", "face"]:
        raise ValueError(f"{path}: expected the elements vertex and face")
    (_, V, vprops), (_, F, fprops) = elements
    names = [p[1] for p in vprops]
    want = ["x", "y", "z"]
    has_color = names == want + ["red", "green", "blue"]
    if not (names == want or has_color) or fprops != [["list", "uchar", "int", "vertex_indices"]]:
        raise ValueError(f"{path}: not the layout write_mesh_ply writes")
    vdt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + ([("red", "u1"), ("green", "u1"), ("blue", "u1")] if has_color else []))
    fdt = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    if len(body) != V * vdt.itemsize + F * fdt.itemsize:
        raise ValueError(f"{path}: truncated, or faces that are not triangles")
    vrec = np.frombuffer(body, vdt, V)
    frec = np.frombuffer(body, fdt, F, offset=V * vdt.itemsize)
    if F and not (frec["n"] == 3).all():
        raise ValueError(f"{path}: faces that are not triangles")
    verts = torch.from_numpy(np.stack([vrec["x"], vrec["y"], vrec["z"]], axis=1).astype(np.float32))
    faces = torch.from_numpy(frec["v"].astype(np.int32).reshape(-1, 3).copy())
    colors = None
    if has_color:
        colors = torch.from_numpy(np.stack([vrec["red"], vrec["green"], vrec["blue"]], axis=1).astype(np.float32) / 255.0)
    return verts, faces, colors
