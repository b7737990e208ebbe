"""Mesh decimation: vertex clustering on a grid with one quadric-placed representative per cluster (Rossignac-Borrel
clusters, Lindstrom's quadric placement).  Marching tetrahedra leaves about two triangles per surface voxel face; this
brings a mesh down to a face count a viewer, an engine or a texture baker can load.

csrc/meshdecimate_math.h states the rule; in short, for a cell size s:

  cell        c = floor(v / s) per axis in float64, the grid anchored at the world origin
  clusters    the distinct cells in ascending (cz, cy, cx); members in ascending vertex index
  vertex      in float64 relative to the cell centre o: m the mean of the members; A, b the area^2-weighted plane quadrics
              of every (face, corner in the cluster); y solves (A + 1e-3 tr(A) I) y = -(b + A m) (y = 0 when tr(A) is 0 or
              not finite); the vertex is float32(o + clamp(m + y, -s/2, s/2)); the colour is the mean of the members'
  faces       a face maps to its three clusters and is dropped when two coincide; with ``dedupe`` only the smallest
              index of the faces with the same unordered cluster triple survives; survivors keep corner and relative order
  output      the clusters a surviving face refers to, in cluster order; faces re-indexed

``target_faces=N`` picks the cell size from the ladder ``cell_size * 2 ** (i / 4)``, i in [0, 64): i = 0 if that already
gives F' <= N, a ValueError if i = 63 does not, otherwise the bisection of ``choose_ladder_index`` (F' is not strictly
monotone in s; the bisection is the definition).  That is at most 8 probes, each a plan with one read-back of its
counts; on the GPU the chosen plan is issued once more, without a read-back, when it was not the last probe (up to 9
plans).

On HIP tensors the kernels of csrc/meshdecimate.hip are the only route (``gs_mesh_decimate_plan``, one read-back of the
counts, ``gs_mesh_decimate_emit``).  CPU tensors take ``mesh_decimate_torch``, the same rule as torch ops (it also runs on
GPU tensors: tools/mesh_decimate_bench.py measures the kernels against it).  The op carries no gradient."""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import torch
from torch import Tensor

MAX_VERTS = 2 ** 30
MAX_FACES = (2 ** 31 - 1) // 3            # 3 F fits an int (csrc/meshdecimate_math.h)
CELL_LIMIT = 2 ** 30
LADDER = 64
# the words of the kernels' counts (csrc/meshdecimate_math.h)
COUNT_WORDS = 8
VERTS_OUT, FACES_OUT, CLUSTERS, DEGENERATE, DUPLICATES, STATUS = range(6)
STATUS_BAD_FACE, STATUS_BAD_VERTEX = 1, 2


class _Desc(ctypes.Structure):
    """gs_mesh_decimate_desc (include/gsdeblur.h)"""
    _fields_ = [("V", ctypes.c_int), ("F", ctypes.c_int), ("verts", ctypes.c_void_p), ("faces", ctypes.c_void_p),
                ("colors", ctypes.c_void_p), ("cell_size", ctypes.c_double), ("dedupe", ctypes.c_int),
                ("counts", ctypes.c_void_p), ("ws", ctypes.c_void_p), ("ws_bytes", ctypes.c_longlong),
                ("verts_out", ctypes.c_void_p), ("faces_out", ctypes.c_void_p), ("colors_out", ctypes.c_void_p),
                ("cluster_of", ctypes.c_void_p), ("V_out", ctypes.c_int), ("F_out", ctypes.c_int),
                ("stream", ctypes.c_void_p)]


def ladder_size(cell_size: float, i: int) -> float:
    return float(cell_size) * 2.0 ** (i / 4)


def choose_ladder_index(reaches) -> int:
    """reaches(i) -> "the plan at ladder_size(cell_size, i) gives F' <= target".  -> the index the module docstring defines"""
    if reaches(0):
        return 0
    if not reaches(LADDER - 1):
        raise ValueError(f"target_faces is not reached even at {LADDER - 1} quarter-octaves above cell_size")
    lo, hi = 0, LADDER - 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if reaches(mid):
            hi = mid
        else:
            lo = mid
    return hi


def _check(verts, faces, colors, cell_size, target_faces):
    if not isinstance(verts, Tensor) or verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32:
        raise ValueError("verts must be a [V,3] float32 tensor")
    if not isinstance(faces, Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise ValueError("faces must be a [F,3] int32 tensor")
    V, F = int(verts.shape[0]), int(faces.shape[0])
    if V > MAX_VERTS or F > MAX_FACES:
        raise ValueError(f"mesh_decimate takes at most 2^30 vertices and {MAX_FACES} faces")
    if colors is not None and (not isinstance(colors, Tensor) or tuple(colors.shape) != (V, 3) or colors.dtype != torch.float32):
        raise ValueError(f"colors must be a [{V},3] float32 tensor or None")
    for name, t in (("faces", faces), ("colors", colors)):
        if t is not None and t.device != verts.device:
            raise ValueError(f"{name} is on {t.device}, verts on {verts.device}")
    if cell_size is None:
        raise ValueError("cell_size is required (with target_faces it is the finest size tried)")
    s = float(cell_size)
    if not (s > 0.0 and math.isfinite(s)):
        raise ValueError(f"cell_size must be positive and finite, got {cell_size}")
    if target_faces is not None:
        if isinstance(target_faces, bool) or int(target_faces) != target_faces or int(target_faces) < 0:
            raise ValueError(f"target_faces must be None or an integer of at least 0, got {target_faces}")
        if not math.isfinite(ladder_size(s, LADDER - 1)):
            raise ValueError(f"cell_size {cell_size} leaves no room for the ladder of target_faces")
    return V, F, s


def _bad_face_error(V):
    return ValueError(f"faces refer to vertices outside [0, {V})")


def _bad_vertex_error():
    return ValueError("verts hold a coordinate that is not finite or more than 2^30 cells of cell_size from the origin")


def _stats(s, plans, clusters, V, F, V_out, F_out, degenerate, duplicates):
    return {"cell_size": float(s), "plans": int(plans), "clusters": int(clusters), "verts_in": int(V), "faces_in": int(F),
            "verts_out": int(V_out), "faces_out": int(F_out), "degenerate": int(degenerate), "duplicates": int(duplicates)}


def _result(mesh, cluster_of, stats, return_map, return_stats):
    out = tuple(mesh)
    if return_map:
        out += (cluster_of,)
    if return_stats:
        out += (stats,)
    return out


def _empty(dev, V, F, color, s, return_map, return_stats):
    mesh = (torch.zeros(0, 3, dtype=torch.float32, device=dev), torch.zeros(0, 3, dtype=torch.int32, device=dev),
            torch.zeros(0, 3, dtype=torch.float32, device=dev) if color else None)
    return _result(mesh, torch.full((V,), -1, dtype=torch.int32, device=dev), _stats(s, 0, 0, V, F, 0, 0, 0, 0),
                   return_map, return_stats)


# --------------------------------------------------------------------------- #
# torch route
# --------------------------------------------------------------------------- #
def _torch_plan(verts: Tensor, faces: Tensor, s: float, dedupe: bool):
    """everything that decides the output sizes, as torch ops -> dict"""
    V, F = verts.shape[0], faces.shape[0]
    q = verts.double() / s
    if not bool(torch.isfinite(q).all()):
        raise _bad_vertex_error()
    cells = torch.floor(q)
    if bool((cells.abs() > CELL_LIMIT).any()):
        raise _bad_vertex_error()
    f = faces.long()
    if bool(((f < 0) | (f >= V)).any()):
        raise _bad_face_error(V)
    cells = cells.long()
    unique, cluster = torch.unique(cells.flip(1), dim=0, return_inverse=True)       # rows (cz, cy, cx), ascending
    C = unique.shape[0]
    tri = cluster[f]
    degenerate = (tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2]) | (tri[:, 0] == tri[:, 2])
    keep = ~degenerate
    duplicates = 0
    if dedupe and bool(keep.any()):
        index = torch.nonzero(keep).reshape(-1)
        canonical = torch.sort(tri[index], dim=1).values
        _, group = torch.unique(canonical, dim=0, return_inverse=True)
        first = torch.full((int(group.max()) + 1,), F, dtype=torch.long, device=verts.device)
        first.scatter_reduce_(0, group, index, "amin")
        survivor = first[group] == index
        duplicates = int((~survivor).sum())
        keep = torch.zeros_like(keep)
        keep[index[survivor]] = True
    ref = torch.zeros(C, dtype=torch.bool, device=verts.device)
    ref[tri[keep].reshape(-1)] = True
    return {"s": s, "cells": unique.flip(1), "cluster": cluster, "tri": tri, "keep": keep, "ref": ref, "clusters": C,
            "faces_out": int(keep.sum()), "verts_out": int(ref.sum()), "degenerate": int(degenerate.sum()),
            "duplicates": duplicates}


def _torch_emit(verts: Tensor, faces: Tensor, colors: Optional[Tensor], plan):
    s, cluster, C, dev = plan["s"], plan["cluster"], plan["clusters"], verts.device
    vd, f = verts.double(), faces.long()
    centre = (plan["cells"].double() + 0.5) * s
    count = torch.bincount(cluster, minlength=C).double().unsqueeze(1)
    m = torch.zeros(C, 3, dtype=torch.float64, device=dev).index_add_(0, cluster, vd - centre[cluster]) / count
    A = torch.zeros(C, 3, 3, dtype=torch.float64, device=dev)
    b = torch.zeros(C, 3, dtype=torch.float64, device=dev)
    for k in range(3):
        ck = cluster[f[:, k]]
        p0, p1, p2 = (vd[f[:, j]] - centre[ck] for j in range(3))
        n = torch.linalg.cross(p1 - p0, p2 - p0)
        d = -(n * p0).sum(1, keepdim=True)
        A.index_add_(0, ck, n.unsqueeze(2) * n.unsqueeze(1))
        b.index_add_(0, ck, d * n)
    trace = A.diagonal(dim1=1, dim2=2).sum(1)
    solvable = torch.isfinite(trace) & (trace != 0)
    eye = torch.eye(3, dtype=torch.float64, device=dev)
    M = torch.where(solvable[:, None, None], A + (1e-3 * trace)[:, None, None] * eye, eye.expand(C, 3, 3))
    rhs = torch.where(solvable[:, None], -(b + (A * m.unsqueeze(1)).sum(2)), torch.zeros_like(b))
    y = torch.linalg.solve(M, rhs.unsqueeze(2)).squeeze(2)
    y = torch.where(torch.isfinite(y).all(1, keepdim=True), y, torch.zeros_like(y))
    x = torch.minimum(torch.maximum(m + y, torch.full_like(m, -0.5 * s)), torch.full_like(m, 0.5 * s))
    ref = plan["ref"]
    new_index = (torch.cumsum(ref.long(), 0) - 1)
    verts_out = (centre + x)[ref].float()
    colors_out = None
    if colors is not None:
        colors_out = (torch.zeros(C, 3, dtype=torch.float64, device=dev).index_add_(0, cluster, colors.double()) / count)[ref].float()
    faces_out = new_index[plan["tri"][plan["keep"]]].to(torch.int32).reshape(-1, 3)
    cluster_of = torch.where(ref[cluster], new_index[cluster], torch.full_like(cluster, -1)).to(torch.int32)
    return (verts_out, faces_out, colors_out), cluster_of


def mesh_decimate_torch(verts: Tensor, faces: Tensor, colors: Optional[Tensor] = None, cell_size: Optional[float] = None,
                        target_faces: Optional[int] = None, dedupe: bool = True, return_map: bool = False,
                        return_stats: bool = False):
    """mesh_decimate as torch ops on verts' device (result as mesh_decimate)"""
    V, F, s = _check(verts, faces, colors, cell_size, target_faces)
    dev = verts.device
    if V == 0 or F == 0:
        return _empty(dev, V, F, colors is not None, s, return_map, return_stats)
    verts, faces = verts.detach(), faces.detach()
    plans = {}

    def plan_at(i):
        if i not in plans:
            plans[i] = _torch_plan(verts, faces, ladder_size(s, i), bool(dedupe))
        return plans[i]
    if target_faces is None:
        chosen = 0
        plan_at(0)
    else:
        chosen = choose_ladder_index(lambda i: plan_at(i)["faces_out"] <= int(target_faces))
    plan = plans[chosen]
    mesh, cluster_of = _torch_emit(verts, faces, None if colors is None else colors.detach(), plan)
    stats = _stats(plan["s"], len(plans), plan["clusters"], V, F, plan["verts_out"], plan["faces_out"], plan["degenerate"],
                   plan["duplicates"])
    return _result(mesh, cluster_of, stats, return_map, return_stats)


# --------------------------------------------------------------------------- #
# HIP route
# --------------------------------------------------------------------------- #
class _Run:
    """one decimation on the GPU: the workspace, the counts and the descriptor; plan(s) and emit()"""

    def __init__(self, verts: Tensor, faces: Tensor, colors: Optional[Tensor], dedupe: bool):
        from . import _lib
        self.lib, self.check = _lib.load(), _lib.check
        self.dev = verts.device
        self.verts, self.faces = verts.detach().contiguous(), faces.detach().contiguous()
        self.colors = None if colors is None else colors.detach().contiguous()
        self.V, self.F = int(verts.shape[0]), int(faces.shape[0])
        self.ws_bytes = int(self.lib.gs_mesh_decimate_workspace_bytes(self.V, self.F))
        if self.ws_bytes < 0:
            raise _lib.HipLibraryError(f"mesh_decimate: unsupported sizes V = {self.V}, F = {self.F}")
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=self.dev)
        self.counts = torch.empty(COUNT_WORDS, dtype=torch.int32, device=self.dev)
        d = self.desc = _Desc()
        d.V, d.F, d.dedupe = self.V, self.F, 1 if dedupe else 0
        d.verts, d.faces = self.verts.data_ptr(), self.faces.data_ptr()
        d.colors = None if self.colors is None else self.colors.data_ptr()
        d.counts, d.ws, d.ws_bytes = self.counts.data_ptr(), self.ws.data_ptr(), self.ws_bytes
        self.plans = 0

    def _call(self, fn, what):
        """the stream current on the mesh's device at EACH launch, never one remembered from construction: the buffers
        and the read-backs are torch's, on the current stream, and every launch goes where they are"""
        self.desc.stream = torch.cuda.current_stream(self.dev).cuda_stream
        self.check(fn(ctypes.c_void_p(ctypes.addressof(self.desc))), what)

    def issue_plan(self, s: float):
        self.desc.cell_size = s
        self._call(self.lib.gs_mesh_decimate_plan, "mesh_decimate plan")

    def plan(self, s: float):
        """one plan and the one read-back of its counts; the status word becomes the error it stands for"""
        from . import _lib
        self.issue_plan(s)
        self.plans += 1
        c = self.counts.tolist()
        if c[STATUS] == STATUS_BAD_FACE:
            raise _bad_face_error(self.V)
        if c[STATUS] == STATUS_BAD_VERTEX:
            raise _bad_vertex_error()
        if c[STATUS] != 0:
            raise _lib.HipLibraryError(f"mesh_decimate: status {c[STATUS]}")
        return c

    def emit(self, c):
        """the outputs of the plan that the workspace holds, for the sizes read back"""
        V_out, F_out, dev = c[VERTS_OUT], c[FACES_OUT], self.dev
        verts_out = torch.empty(V_out, 3, dtype=torch.float32, device=dev)
        faces_out = torch.empty(F_out, 3, dtype=torch.int32, device=dev)
        colors_out = None if self.colors is None else torch.empty(V_out, 3, dtype=torch.float32, device=dev)
        cluster_of = torch.empty(self.V, dtype=torch.int32, device=dev)
        d = self.desc
        d.V_out, d.F_out = V_out, F_out
        d.verts_out = verts_out.data_ptr() if V_out else None
        d.faces_out = faces_out.data_ptr() if F_out else None
        d.colors_out = colors_out.data_ptr() if colors_out is not None and V_out else None
        d.cluster_of = cluster_of.data_ptr()
        self._call(self.lib.gs_mesh_decimate_emit, "mesh_decimate emit")
        return (verts_out, faces_out, colors_out), cluster_of


def mesh_decimate_hip(verts: Tensor, faces: Tensor, colors: Optional[Tensor] = None, cell_size: Optional[float] = None,
                      target_faces: Optional[int] = None, dedupe: bool = True, return_map: bool = False,
                      return_stats: bool = False):
    """the kernels of csrc/meshdecimate.hip on GPU tensors (result as mesh_decimate)"""
    V, F, s = _check(verts, faces, colors, cell_size, target_faces)
    if not verts.is_cuda:
        raise ValueError("verts must be a CUDA(HIP) tensor: the HIP path has no CPU fallback")
    dev = verts.device
    if V == 0 or F == 0:
        return _empty(dev, V, F, colors is not None, s, return_map, return_stats)
    with torch.cuda.device(dev):
        run = _Run(verts, faces, colors, bool(dedupe))
        seen, last = {}, [None]

        def plan_at(i):
            if i not in seen:
                seen[i] = run.plan(ladder_size(s, i))
                last[0] = i
            return seen[i]
        if target_faces is None:
            chosen = 0
            plan_at(0)
        else:
            chosen = choose_ladder_index(lambda i: plan_at(i)[FACES_OUT] <= int(target_faces))
        c = seen[chosen]
        if last[0] != chosen:
            run.issue_plan(ladder_size(s, chosen))      # the workspace holds a later probe: the chosen plan again, sizes known
        mesh, cluster_of = run.emit(c)
    stats = _stats(ladder_size(s, chosen), run.plans, c[CLUSTERS], V, F, c[VERTS_OUT], c[FACES_OUT], c[DEGENERATE],
                   c[DUPLICATES])
    return _result(mesh, cluster_of, stats, return_map, return_stats)


# --------------------------------------------------------------------------- #
# public
# --------------------------------------------------------------------------- #
def mesh_decimate(verts: Tensor, faces: Tensor, colors: Optional[Tensor] = None, cell_size: Optional[float] = None,
                  target_faces: Optional[int] = None, dedupe: bool = True, return_map: bool = False,
                  return_stats: bool = False):
    """Decimate a triangle mesh by vertex clustering (module docstring: the rule) -> (verts' [V',3] float32, faces' [F',3]
    int32, colors' [V',3] float32 or None), with return_map also cluster_of [V] int32 (the output vertex of every input
    vertex, -1 where its cluster was dropped) and with return_stats a dict: cell_size (the one used), plans (the probes:
    plans whose counts were read back), clusters, verts_in, verts_out, faces_in, faces_out, degenerate, duplicates.
    verts [V,3] float32, faces [F,3] int32, colors [V,3] float32 or None, all on one device.  cell_size is required; with
    target_faces=N it is the finest size of the ladder and the first size the bisection accepts (F' <= N) is used.  A face
    index outside [0, V), a coordinate that is not finite or more than 2^30 cells from the origin, and a target no ladder
    size reaches are ValueErrors.  V == 0 or F == 0 gives the empty mesh.  HIP tensors take the kernels, CPU tensors
    mesh_decimate_torch.  No gradient."""
    fn = mesh_decimate_hip if isinstance(verts, Tensor) and verts.is_cuda else mesh_decimate_torch
    return fn(verts, faces, colors, cell_size, target_faces, dedupe, return_map, return_stats)
