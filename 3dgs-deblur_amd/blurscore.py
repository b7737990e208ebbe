"""Per-frame blur statistics of a point cloud under the motion model: how blurred will each frame of a capture be?

For frame f and point p (csrc/blur_math.h states every operation): the point's camera-space position pc = V_f p, its
pixel (u, v), its pixel velocity pv — the renderer's own first-order formula, ``pixel_velocity`` of csrc/gs_math.h, from
the camera's body twist — and from it ``blur = E_f |pv|``, the length in pixels of the streak the exposure draws, and
``skew = T_f |pv| |v / H - 1/2|``, how far the rolling shutter displaces the point's row.  A pair counts when the point is
in front of the clip plane and inside the image.  Per frame, over the pairs that count: their number, the mean, root mean
square and maximum of blur, and the mean of skew; zeros for a frame that sees no point.

``mean_blur`` is what the reference's datasets call ``motion_blur_score`` (there it comes from a proprietary tool):
``data.split_indices(..., scores=)`` picks the sharpest frame of every run of frames for evaluation with it.

Per-pair values are float32 with every operation rounded; the sums are float64 in a fixed order, so two calls agree bit
for bit.  On HIP tensors the kernels of csrc/blur.hip are the only route (``gs_blur_stats``: two launches, no atomics,
nothing read back); CPU tensors take ``blur_stats_torch``, the same operations as torch ops over chunks of frames.  No
gradient."""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Tuple

import torch
from torch import Tensor

DEFAULT_CLIP = 0.01                  # csrc/blur_math.h kDefaultClip: the projection's near plane
CHUNK = 1024                         # kChunk
FRAME_GROUP = 32                     # kFrameGroup
MAX_FRAMES = 65535 * FRAME_GROUP
MAX_POINTS = 1 << 30
_CHUNK_ELEMS = 1 << 21               # blur_stats_torch: frames x N pairs per chunk


class BlurStats(NamedTuple):
    """per frame, over its visible (frame, point) pairs; all [F]"""
    count: Tensor        # int32
    mean_blur: Tensor    # float32, pixels
    rms_blur: Tensor
    max_blur: Tensor
    mean_skew: Tensor


def _check(points, viewmats, lin_vel, ang_vel, intrins, times, W, H, clip) -> Tuple[int, int]:
    ts = (points, viewmats, lin_vel, ang_vel, intrins, times)
    for name, t in zip(("points", "viewmats", "lin_vel", "ang_vel", "intrins", "times"), ts):
        if not isinstance(t, Tensor) or t.dtype != torch.float32:
            raise ValueError(f"{name} must be a float32 tensor")
        if t.device != points.device:
            raise ValueError(f"{name} is on {t.device}, points on {points.device}")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be [N,3], got {tuple(points.shape)}")
    F = int(viewmats.shape[0])
    if tuple(viewmats.shape) != (F, 4, 4):
        raise ValueError(f"viewmats must be [F,4,4], got {tuple(viewmats.shape)}")
    for name, t, w in (("lin_vel", lin_vel, 3), ("ang_vel", ang_vel, 3), ("intrins", intrins, 4), ("times", times, 2)):
        if tuple(t.shape) != (F, w):
            raise ValueError(f"{name} must be [{F},{w}], got {tuple(t.shape)}")
    if int(W) < 1 or int(H) < 1:
        raise ValueError(f"the image must be at least 1 x 1, got {W} x {H}")
    if not float(clip) == float(clip):
        raise ValueError("clip must be a number")
    N = int(points.shape[0])
    if F > MAX_FRAMES or N > MAX_POINTS:
        raise ValueError(f"blur_stats supports at most {MAX_FRAMES} frames and {MAX_POINTS} points, got {F} and {N}")
    return F, N


# --------------------------------------------------------------------------- #
# HIP
# --------------------------------------------------------------------------- #
def blur_stats_hip(points: Tensor, viewmats: Tensor, lin_vel: Tensor, ang_vel: Tensor, intrins: Tensor, times: Tensor,
                   W: int, H: int, clip: float = DEFAULT_CLIP, points_per_thread: int = 0,
                   workspace_bytes: int = -1) -> BlurStats:
    """gs_blur_stats on GPU tensors.  points_per_thread (1, 2, 4, 8, 16; 0: the library's choice) is the tuning knob of
    tools/blur_score_bench.py; workspace_bytes >= 0 hands the call a workspace of that size instead of the one it asks
    for (tests)."""
    from . import _lib
    if not points.is_cuda:
        raise ValueError("points must be a CUDA(HIP) tensor: the HIP path has no CPU fallback")
    F, N = _check(points, viewmats, lin_vel, ang_vel, intrins, times, W, H, clip)
    dev = points.device
    points, viewmats, lin_vel, ang_vel, intrins, times = (t.detach().contiguous() for t in
                                                          (points, viewmats, lin_vel, ang_vel, intrins, times))
    counts = torch.empty(F, dtype=torch.int32, device=dev)
    stats = torch.empty(F, 4, dtype=torch.float32, device=dev)
    lib = _lib.load()
    vp = ctypes.c_void_p
    with torch.cuda.device(dev):
        ws_bytes = int(lib.gs_blur_stats_workspace_bytes(F, N)) if workspace_bytes < 0 else int(workspace_bytes)
        if ws_bytes < 0:
            raise _lib.HipLibraryError(f"blur_stats: unsupported shape F={F}, N={N}")
        ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=dev)
        _lib.check(lib.gs_blur_stats_ppt(F, N, vp(points.data_ptr()), vp(viewmats.data_ptr()), vp(lin_vel.data_ptr()),
                                         vp(ang_vel.data_ptr()), vp(intrins.data_ptr()), vp(times.data_ptr()), int(W),
                                         int(H), float(clip), int(points_per_thread), vp(counts.data_ptr()),
                                         vp(stats.data_ptr()), vp(ws.data_ptr()), ws_bytes,
                                         vp(torch.cuda.current_stream().cuda_stream)), "blur_stats")
    return BlurStats(counts, stats[:, 0].contiguous(), stats[:, 1].contiguous(), stats[:, 2].contiguous(),
                     stats[:, 3].contiguous())


# --------------------------------------------------------------------------- #
# torch restatement (CPU tensors)
# --------------------------------------------------------------------------- #
def blur_stats_torch(points: Tensor, viewmats: Tensor, lin_vel: Tensor, ang_vel: Tensor, intrins: Tensor, times: Tensor,
                     W: int, H: int, clip: float = DEFAULT_CLIP) -> BlurStats:
    """the same statistics as torch ops on the tensors' device: the operations of csrc/blur_math.h one by one in float32
    (a product and a sum are two roundings in torch), the sums in float64; frames x N values at a time for at most
    2^21 / N frames, so memory stays linear in N"""
    F, N = _check(points, viewmats, lin_vel, ang_vel, intrins, times, W, H, clip)
    dev = points.device
    points, viewmats, lin_vel, ang_vel, intrins, times = (t.detach() for t in
                                                          (points, viewmats, lin_vel, ang_vel, intrins, times))
    count = torch.zeros(F, dtype=torch.int32, device=dev)
    out = torch.zeros(4, F, dtype=torch.float32, device=dev)
    if F == 0 or N == 0:
        return BlurStats(count, out[0], out[1], out[2], out[3])
    px, py, pz = (points[None, :, a] for a in range(3))
    Wf, Hf, clipf = (torch.tensor(float(v), dtype=torch.float32, device=dev) for v in (W, H, clip))
    rows = max(1, _CHUNK_ELEMS // N)
    for lo in range(0, F, rows):
        hi = min(F, lo + rows)
        V = viewmats[lo:hi].reshape(hi - lo, 16)
        v = [V[:, k, None] for k in range(12)]
        lin, ang = ([t[lo:hi, a, None] for a in range(3)] for t in (lin_vel, ang_vel))
        fx, fy, cx, cy = (intrins[lo:hi, a, None] for a in range(4))
        E, T = times[lo:hi, 0, None], times[lo:hi, 1, None]
        pcx = ((v[0] * px + v[1] * py) + v[2] * pz) + v[3]
        pcy = ((v[4] * px + v[5] * py) + v[6] * pz) + v[7]
        pcz = ((v[8] * px + v[9] * py) + v[10] * pz) + v[11]
        rz = 1.0 / pcz
        u = (fx * pcx) * rz + cx
        vv = (fy * pcy) * rz + cy
        # pixel_velocity (csrc/gs_math.h) with jx = pc.x, jy = pc.y
        ux = -(ang[1] * pcz - ang[2] * pcy) - lin[0]
        uy = -(ang[2] * pcx - ang[0] * pcz) - lin[1]
        uz = -(ang[0] * pcy - ang[1] * pcx) - lin[2]
        rz2 = rz * rz
        pvx = (fx * rz) * ux - ((fx * pcx) * rz2) * uz
        pvy = (fy * rz) * uy - ((fy * pcy) * rz2) * uz
        mag = (pvx * pvx + pvy * pvy).double().sqrt().float()      # the correctly rounded float32 root
        blur = E * mag
        skew = (T * mag) * torch.abs(vv / Hf - 0.5)
        vis = (pcz > clipf) & (u >= 0) & (u < Wf) & (vv >= 0) & (vv < Hf)
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        b = torch.where(vis, blur.double(), zero)
        n = vis.sum(dim=1)
        nd = n.clamp(min=1).double()
        some = n > 0
        count[lo:hi] = n.to(torch.int32)
        out[0, lo:hi] = torch.where(some, b.sum(dim=1) / nd, zero).float()
        out[1, lo:hi] = torch.where(some, torch.sqrt((b * b).sum(dim=1) / nd), zero).float()
        out[2, lo:hi] = torch.where(vis, blur, torch.zeros((), dtype=torch.float32, device=dev)).amax(dim=1)
        out[3, lo:hi] = torch.where(some, torch.where(vis, skew.double(), zero).sum(dim=1) / nd, zero).float()
    return BlurStats(count, out[0], out[1], out[2], out[3])


# --------------------------------------------------------------------------- #
# public surface
# --------------------------------------------------------------------------- #
def blur_stats(points: Tensor, viewmats: Tensor, lin_vel: Tensor, ang_vel: Tensor, intrins: Tensor, times: Tensor,
               W: int, H: int, clip: float = DEFAULT_CLIP) -> BlurStats:
    """BlurStats(count, mean_blur, rms_blur, max_blur, mean_skew), each [F], of points [N,3] seen by F frames (module
    docstring): viewmats [F,4,4] world-to-camera in OpenCV axes, lin_vel / ang_vel [F,3] the camera's body twist in that
    frame (view_and_twist converts a dataset's OpenGL pose and velocities), intrins [F,4] = fx fy cx cy, times [F,2] =
    exposure and readout in seconds; all float32 on one device.  W, H: the image size that decides visibility, clip: the
    near plane.  ValueError for a wrong shape, dtype or device.  No gradient."""
    if not isinstance(points, Tensor):
        raise ValueError("points must be a tensor")
    if points.is_cuda:
        return blur_stats_hip(points, viewmats, lin_vel, ang_vel, intrins, times, W, H, clip)
    return blur_stats_torch(points, viewmats, lin_vel, ang_vel, intrins, times, W, H, clip)


def view_and_twist(c2w: Tensor, lin_vel: Tensor, ang_vel: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """a dataset's camera — camera_to_world [..., 3 or 4, 4] in OpenGL axes (x right, y up, z back) and velocities [..., 3] in
    that camera frame, as transforms.json stores them — in the kernels' convention: (world-to-camera [..., 4, 4] in OpenCV
    axes, linear and angular velocity [..., 3] in that frame).  The y and z axes change sign; dtype and device are kept."""
    flip = torch.tensor([1.0, -1.0, -1.0], dtype=c2w.dtype, device=c2w.device)
    R_wc = (c2w[..., :3, :3] * flip).transpose(-1, -2)
    t_wc = -(R_wc @ c2w[..., :3, 3:4])
    bottom = torch.zeros(c2w.shape[:-2] + (1, 4), dtype=c2w.dtype, device=c2w.device)
    bottom[..., 0, 3] = 1.0
    viewmat = torch.cat([torch.cat([R_wc, t_wc], dim=-1), bottom], dim=-2)
    return viewmat, lin_vel * flip.to(lin_vel.dtype), ang_vel * flip.to(ang_vel.dtype)

