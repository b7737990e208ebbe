"""Mesh clean-up: the connected components of a triangle mesh and the removal of the small ones (the floaters a splat
model leaves in a TSDF volume come out of ``tsdf_extract_mesh`` as closed little islands).

The graph has the V vertices as nodes and the three sides of every face as edges.  ``labels[v]`` is the smallest vertex
index of v's component, a pure function of the mesh; a vertex no face refers to is a component with 0 faces; a face
belongs to the component of its vertices.  csrc/meshclean_math.h states the rounds and the filter rule; in short:

  rounds   parent[v] = v; a round hooks (for every side (a, b): the larger of the two roots gets the smaller as parent, by
           min) and compresses (parent[v] = root(v)); the first round that hooks nothing ends the loop
  filter   rank the components with at least one face by (face count descending, label ascending); ``keep_largest=K``
           lets only the first min(K, C) through (strict: ties go to the smaller label); of these the ones with fewer than
           ``min_faces`` faces are dropped; components with 0 faces are always dropped; surviving vertices and faces keep
           their relative order, faces are re-indexed

On HIP tensors the kernels of csrc/meshclean.hip are the only route (``gs_mesh_components_round`` with one 4-byte
read-back per round, ``gs_mesh_components_finish``, ``gs_mesh_filter_plan``, one read-back of V', F', C, kept and the
status word, ``gs_mesh_filter_emit``).  CPU tensors take ``mesh_components_torch`` and ``mesh_filter_components_torch``:
the same rounds, every side at once.  Both give the same bits, every run."""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch
from torch import Tensor

MAX_COUNT = 2 ** 31 - 1
# the words of the kernels' counts (csrc/meshclean_math.h)
COUNT_WORDS = 8
VERTS_OUT, FACES_OUT, COMPONENTS, KEPT, STATUS, HOOKED_ROUND = range(6)
STATUS_BAD_FACE, STATUS_BAD_LABEL = 1, 2


def max_rounds(num_verts: int) -> int:
    """the rounds a correct run stays far inside (meshclean_math.h max_rounds): more than that shows a defect"""
    return 8 * int(num_verts).bit_length() + 8


def _check_faces(faces, num_verts):
    if not isinstance(faces, Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise ValueError("faces must be a [F,3] int32 tensor")
    V = int(num_verts)
    if V < 0 or V > MAX_COUNT or faces.shape[0] > MAX_COUNT:
        raise ValueError("a mesh holds at most 2^31 - 1 vertices and faces")
    return V, int(faces.shape[0])


def _check_filter(verts, faces, colors, min_faces, keep_largest):
    if not isinstance(verts, Tensor) or verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32:
        raise ValueError("verts must be a [V,3] float32 tensor")
    V, F = _check_faces(faces, verts.shape[0])
    if colors is not None and (not isinstance(colors, Tensor) or tuple(colors.shape) != (V, 3) or colors.dtype != torch.float32):
        raise ValueError(f"colors must be a [{V},3] float32 tensor or None")
    for name, t in (("faces", faces), ("colors", colors)):
        if t is not None and t.device != verts.device:
            raise ValueError(f"{name} is on {t.device}, verts on {verts.device}")
    if int(min_faces) < 0:
        raise ValueError(f"min_faces must be at least 0, got {min_faces}")
    if keep_largest is not None and int(keep_largest) < 1:
        raise ValueError(f"keep_largest must be None or at least 1, got {keep_largest}")
    return V, F


def _bad_face_error(V):
    return ValueError(f"faces refer to vertices outside [0, {V})")


def _empty_mesh(dev, color: bool):
    return (torch.zeros(0, 3, dtype=torch.float32, device=dev), torch.zeros(0, 3, dtype=torch.int32, device=dev),
            torch.zeros(0, 3, dtype=torch.float32, device=dev) if color else None)


def _stats(components, kept, rounds, V, F, V_out, F_out):
    return {"components": int(components), "kept": int(kept), "rounds": int(rounds), "verts_in": int(V), "faces_in": int(F),
            "verts_out": int(V_out), "faces_out": int(F_out)}


# --------------------------------------------------------------------------- #
# CPU route
# --------------------------------------------------------------------------- #
def _rounds_numpy(faces: np.ndarray, V: int):
    """the rounds of meshclean_math.h with every side of a round hooked at once -> (labels [V] int32, rounds)"""
    parent = np.arange(V, dtype=np.int32)
    a = faces.reshape(-1)
    b = faces[:, (1, 2, 0)].reshape(-1)
    rounds, guard = 0, max_rounds(V)
    while True:
        if rounds >= guard:
            from ._lib import HipLibraryError
            raise HipLibraryError(f"mesh_components: no fixed point after {rounds} rounds")
        rounds += 1
        ra, rb = parent[a], parent[b]                  # parent is compressed here: these are the roots
        differ = ra != rb
        if not differ.any():
            return parent, rounds
        np.minimum.at(parent, np.maximum(ra, rb)[differ], np.minimum(ra, rb)[differ])
        while True:
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up


def _table_numpy(labels: np.ndarray, faces: np.ndarray):
    V = len(labels)
    roots = np.flatnonzero(labels == np.arange(V, dtype=np.int32)).astype(np.int32)
    face_counts = np.bincount(labels[faces[:, 0]], minlength=V)[roots].astype(np.int32) if len(faces) else np.zeros(len(roots), np.int32)
    vert_counts = np.bincount(labels, minlength=V)[roots].astype(np.int32)
    return roots, face_counts, vert_counts


def _faces_numpy(faces: Tensor, V: int) -> np.ndarray:
    f = faces.detach().cpu().numpy()
    if len(f) and (f.min() < 0 or f.max() >= V):
        raise _bad_face_error(V)
    return f


def mesh_components_torch(faces: Tensor, num_verts: int, return_table: bool = False, _return_rounds: bool = False):
    """mesh_components on the host (result as mesh_components, on faces' device)"""
    V, F = _check_faces(faces, num_verts)
    dev = faces.device
    f = _faces_numpy(faces, V)
    labels, rounds = _rounds_numpy(f, V) if F and V else (np.arange(V, dtype=np.int32), 0)
    out = [torch.from_numpy(labels).to(dev)]
    if return_table:
        out += [torch.from_numpy(t).to(dev) for t in _table_numpy(labels, f)]
    if _return_rounds:
        out.append(rounds)
    return out[0] if len(out) == 1 else tuple(out)


def mesh_filter_components_torch(verts: Tensor, faces: Tensor, colors: Optional[Tensor] = None, min_faces: int = 1,
                                 keep_largest: Optional[int] = None, return_stats: bool = False):
    """mesh_filter_components on the host (result as mesh_filter_components, on verts' device)"""
    V, F = _check_filter(verts, faces, colors, min_faces, keep_largest)
    dev = verts.device
    f = _faces_numpy(faces, V)
    if V == 0 or F == 0:
        mesh = _empty_mesh(dev, colors is not None)
        return mesh + (_stats(V, 0, 0, V, F, 0, 0),) if return_stats else mesh
    labels, rounds = _rounds_numpy(f, V)
    roots, face_counts, _ = _table_numpy(labels, f)
    ranked = np.flatnonzero(face_counts >= 1)
    ranked = ranked[np.lexsort((roots[ranked], -face_counts[ranked].astype(np.int64)))]
    if keep_largest is not None:
        ranked = ranked[:int(keep_largest)]
    ranked = ranked[face_counts[ranked] >= int(min_faces)]
    keep_root = np.zeros(V, bool)
    keep_root[roots[ranked]] = True
    keep_v = keep_root[labels]
    keep_f = keep_v[f[:, 0]]
    new_index = (np.cumsum(keep_v) - 1).astype(np.int32)
    kv, kf = torch.from_numpy(keep_v), torch.from_numpy(keep_f)
    verts_out = verts.detach().cpu()[kv].to(dev)
    colors_out = None if colors is None else colors.detach().cpu()[kv].to(dev)
    faces_out = torch.from_numpy(new_index[f[keep_f]].reshape(-1, 3)).to(dev)
    mesh = (verts_out, faces_out, colors_out)
    if return_stats:
        mesh += (_stats(len(roots), len(ranked), rounds, V, F, int(keep_v.sum()), int(keep_f.sum())),)
    return mesh


# --------------------------------------------------------------------------- #
# HIP route
# --------------------------------------------------------------------------- #
class _Run:
    """one labelling on the GPU: the rounds and gs_mesh_components_finish are issued, counts is not read back yet"""

    def __init__(self, faces: Tensor, V: int, what: str):
        from . import _lib
        self.lib, self.check, self.what = _lib.load(), _lib.check, what
        self.V, self.F, self.dev = V, int(faces.shape[0]), faces.device
        self.faces = faces.detach().contiguous()
        vp = ctypes.c_void_p
        self.ws_bytes = int(self.lib.gs_mesh_clean_workspace_bytes(V, self.F))
        if self.ws_bytes < 0:
            raise _lib.HipLibraryError(f"{what}: unsupported sizes V = {V}, F = {self.F}")
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=self.dev)
        self.labels = torch.empty(V, dtype=torch.int32, device=self.dev)
        self.counts = torch.empty(COUNT_WORDS, dtype=torch.int32, device=self.dev)
        self.p_faces, self.p_labels, self.p_counts = vp(self.faces.data_ptr()), vp(self.labels.data_ptr()), vp(self.counts.data_ptr())
        self.p_ws = vp(self.ws.data_ptr())
        self.rounds, guard = 0, max_rounds(V)
        while True:
            if self.rounds >= guard:
                raise _lib.HipLibraryError(f"{what}: no fixed point after {self.rounds} rounds")
            self.check(self.lib.gs_mesh_components_round(V, self.F, self.p_faces, self.p_labels, self.rounds, self.p_counts,
                                                         self.stream), what + " round")
            self.rounds += 1
            if int(self.counts[HOOKED_ROUND].item()) != self.rounds:          # the 4-byte read-back of the round
                break
        self.check(self.lib.gs_mesh_components_finish(V, self.F, self.p_faces, self.p_labels, self.p_counts, self.p_ws,
                                                      self.ws_bytes, self.stream), what + " finish")

    @property
    def stream(self):
        """the stream current on the mesh's device at EACH launch, never one remembered from construction: the run's
        buffers and read-backs are torch's, on the current stream, and every launch goes where they are"""
        return ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def read_counts(self):
        """the one read-back of the final counts; the status word becomes the error it stands for"""
        from . import _lib
        c = self.counts.tolist()
        if c[STATUS] == STATUS_BAD_FACE:
            raise _bad_face_error(self.V)
        if c[STATUS] != 0:
            raise _lib.HipLibraryError(f"{self.what}: status {c[STATUS]}")
        return c


def mesh_components_hip(faces: Tensor, num_verts: int, return_table: bool = False):
    """the kernels of csrc/meshclean.hip on a GPU tensor (result as mesh_components)"""
    V, F = _check_faces(faces, num_verts)
    if not faces.is_cuda:
        raise ValueError("faces must be a CUDA(HIP) tensor: the HIP path has no CPU fallback")
    dev = faces.device
    if V == 0 or F == 0:
        labels = torch.arange(V, dtype=torch.int32, device=dev)
        if not return_table:
            return labels
        return labels, labels.clone(), torch.zeros(V, dtype=torch.int32, device=dev), torch.ones(V, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        run = _Run(faces, V, "mesh_components")
        C = run.read_counts()[COMPONENTS]
        if not return_table:
            return run.labels
        roots, face_counts, vert_counts = (torch.empty(C, dtype=torch.int32, device=dev) for _ in range(3))
        vp = ctypes.c_void_p
        run.check(run.lib.gs_mesh_components_table(V, F, C, vp(roots.data_ptr()), vp(face_counts.data_ptr()),
                                                   vp(vert_counts.data_ptr()), run.p_ws, run.ws_bytes, run.stream),
                  "mesh_components table")
    return run.labels, roots, face_counts, vert_counts


def mesh_filter_components_hip(verts: Tensor, faces: Tensor, colors: Optional[Tensor] = None, min_faces: int = 1,
                               keep_largest: Optional[int] = None, return_stats: bool = False):
    """the kernels of csrc/meshclean.hip on GPU tensors (result as mesh_filter_components)"""
    V, F = _check_filter(verts, faces, colors, min_faces, keep_largest)
    if not verts.is_cuda:
        raise ValueError("verts must be a CUDA(HIP) tensor: the HIP path has no CPU fallback")
    dev = verts.device
    if V == 0 or F == 0:
        mesh = _empty_mesh(dev, colors is not None)
        return mesh + (_stats(V, 0, 0, V, F, 0, 0),) if return_stats else mesh
    vp = ctypes.c_void_p
    verts = verts.detach().contiguous()
    colors = None if colors is None else colors.detach().contiguous()
    with torch.cuda.device(dev):
        run = _Run(faces, V, "mesh_filter_components")
        run.check(run.lib.gs_mesh_filter_plan(V, F, run.p_faces, run.p_labels, min(int(min_faces), MAX_COUNT),
                                              0 if keep_largest is None else min(int(keep_largest), MAX_COUNT), run.p_counts,
                                              run.p_ws, run.ws_bytes, run.stream), "mesh_filter_plan")
        c = run.read_counts()
        V_out, F_out = c[VERTS_OUT], c[FACES_OUT]
        if V_out == 0 and F_out == 0:
            mesh = _empty_mesh(dev, colors is not None)
        else:
            verts_out = torch.empty(V_out, 3, dtype=torch.float32, device=dev)
            faces_out = torch.empty(F_out, 3, dtype=torch.int32, device=dev)
            colors_out = None if colors is None else torch.empty(V_out, 3, dtype=torch.float32, device=dev)
            run.check(run.lib.gs_mesh_filter_emit(V, F, vp(verts.data_ptr()), run.p_faces,
                                                  vp(None if colors is None else colors.data_ptr()), run.p_labels, V_out, F_out,
                                                  vp(verts_out.data_ptr()), vp(faces_out.data_ptr()),
                                                  vp(None if colors_out is None else colors_out.data_ptr()), run.p_ws,
                                                  run.ws_bytes, run.stream), "mesh_filter_emit")
            mesh = (verts_out, faces_out, colors_out)
    if return_stats:
        mesh += (_stats(c[COMPONENTS], c[KEPT], run.rounds, V, F, V_out, F_out),)
    return mesh


# --------------------------------------------------------------------------- #
# public
# --------------------------------------------------------------------------- #
def mesh_components(faces: Tensor, num_verts: int, return_table: bool = False):
    """Connected components of a triangle mesh -> labels [V] int32: labels[v] is the smallest vertex index of v's
    component (module docstring).  faces [F,3] int32; an index outside [0, num_verts) is a ValueError.  With
    return_table also roots [C] int32 ascending, face_counts [C] int32 and vert_counts [C] int32.  HIP tensors take the
    kernels, CPU tensors mesh_components_torch."""
    fn = mesh_components_hip if isinstance(faces, Tensor) and faces.is_cuda else mesh_components_torch
    return fn(faces, num_verts, return_table)


def mesh_filter_components(verts: Tensor, faces: Tensor, colors: Optional[Tensor] = None, min_faces: int = 1,
                           keep_largest: Optional[int] = None, return_stats: bool = False):
    """Remove small components (module docstring: the rule) -> (verts' [V',3] float32, faces' [F',3] int32, colors'
    [V',3] float32 or None), and with return_stats a dict: components (before filtering), kept, rounds, verts_in,
    faces_in, verts_out, faces_out.  verts [V,3] float32, faces [F,3] int32, colors [V,3] float32 (colours or any other
    per-vertex attribute) or None, all on one device.  With the defaults a mesh whose every vertex is referenced comes
    back equal.  HIP tensors take the kernels, CPU tensors mesh_filter_components_torch."""
    fn = mesh_filter_components_hip if isinstance(verts, Tensor) and verts.is_cuda else mesh_filter_components_torch
    return fn(verts, faces, colors, min_faces, keep_largest, return_stats)
