"""`transforms.json` loader: the wire format between the reference's data preparation and the model
(App. B).  Field contract, all from the reference tree:
  top level   w h cx cy fl_x fl_y k1 k2 p1 p2 exposure_time rolling_shutter_time frames[]
              (/root/reference/process_synthetic_inputs.py:113-129), optional ply_file_path (:298),
              applied_transform, k3 (/root/reference/combine.py:118,127)
  per frame   file_path transform_matrix[4][4] camera_linear_velocity[3] camera_angular_velocity[3]
              (/root/reference/process_synthetic_inputs.py:171-176), optional motion_blur_score
              (/root/reference/combine.py:79-81); optional depth_file_path (nerfstudio's depth supervision field;
              top-level depth_unit_scale_factor, default 1e-3: stored value * factor = scene units; load_depth)
  conventions camera-to-world in OpenGL axes; velocities in that camera frame
              (/root/reference/process_synthetic_inputs.py:157-165)
  eval split  "interval": sorted index i % 8 == 0 (/root/reference/train.py:174-177,
              /root/reference/process_synthetic_inputs.py:287-293); "filename": eval_/train_ prefixes
              (/root/reference/train_eval_split_by_blur_score.py:34-37, /root/reference/train.py:169-172);
              "all" (/root/reference/train.py:164-167); "blur_score": the sharpest frame of every run of 8 by
              motion_blur_score, the split /root/reference/train_eval_split_by_blur_score.py:27-47 writes into file names
              (write_blur_scored writes that dataset; blur_scores computes the score the reference takes from sai-cli)
Host code (json + torch tensors); `load_image` decodes the frames (PNG / JPEG through PIL, or .npy float arrays)
and `write_transforms` / `write_seed_points_ply` emit the same wire format (used by the self-generated datasets of
``tools/synthetic_dataset.py``, the offline stand-in for the Zenodo downloads of /root/reference/download_data.py:21-33).
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch

from .model import Camera


NORMAL_CONVENTIONS = ("opencv", "opengl")


@dataclass
class TransformsScene:
    cameras: List[Camera]
    image_paths: List[str]
    train_indices: List[int]
    eval_indices: List[int]
    exposure_time: float
    rolling_shutter_time: float
    distortion: Dict[str, float] = field(default_factory=dict)
    ply_file_path: Optional[str] = None
    applied_transform: Optional[torch.Tensor] = None
    # per frame: the depth map's path (nerfstudio's depth_file_path) or None; [] for scenes built by hand
    depth_paths: List[Optional[str]] = field(default_factory=list)
    depth_unit_scale_factor: float = 1e-3
    # per frame: the normal prior's path (normal_file_path) or None; normal_convention "opencv" (x right, y down, z
    # forward: the frame of normals.depth_normals) or "opengl" (y and z negated on load)
    normal_paths: List[Optional[str]] = field(default_factory=list)
    normal_convention: str = "opencv"


def split_indices(file_paths: List[str], eval_mode: str = "interval", eval_interval: int = 8,
                  scores: Optional[List[float]] = None) -> Tuple[List[int], List[int]]:
    """(train, eval) indices into the path-sorted frame list.  eval_mode "blur_score" (the rule of
    /root/reference/train_eval_split_by_blur_score.py:27-47) cuts the frames into runs of eval_interval — the last may be
    shorter — and takes the frame with the smallest of `scores` (one per frame, in the same order) in each run for
    evaluation, the first of them on a tie; the others train."""
    n = len(file_paths)
    if eval_mode == "all":
        return list(range(n)), list(range(n))
    if eval_mode == "interval":
        ev = [i for i in range(n) if i % eval_interval == 0]
        return [i for i in range(n) if i % eval_interval != 0], ev
    if eval_mode == "filename":
        ev = [i for i, p in enumerate(file_paths) if os.path.basename(p).startswith("eval_")]
        tr = [i for i, p in enumerate(file_paths) if os.path.basename(p).startswith("train_")]
        if not ev and not tr:
            raise ValueError("eval_mode='filename' needs eval_/train_ prefixed file names")
        return tr, ev
    if eval_mode == "blur_score":
        if scores is None or len(scores) != n:
            raise ValueError("eval_mode='blur_score' needs one score per frame")
        if int(eval_interval) < 1:
            raise ValueError("eval_interval must be at least 1")
        ev = [min(range(lo, min(n, lo + eval_interval)), key=lambda i: scores[i]) for lo in range(0, n, eval_interval)]
        chosen = set(ev)
        return [i for i in range(n) if i not in chosen], ev
    raise ValueError(f"unknown eval_mode {eval_mode!r}")


def load_transforms(path: str, eval_mode: str = "interval", eval_interval: int = 8,
                    downscale: int = 1) -> TransformsScene:
    """Parse a nerfstudio-style transforms.json written by the reference's converters."""
    json_path = os.path.join(path, "transforms.json") if os.path.isdir(path) else path
    root = os.path.dirname(json_path)
    with open(json_path, "rt") as f:
        meta = json.load(f)
    for k in ("w", "h", "fl_x", "fl_y", "cx", "cy", "frames"):
        if k not in meta:
            raise KeyError(f"transforms.json misses '{k}'")
    frames = sorted(meta["frames"], key=lambda fr: fr["file_path"])
    exposure = float(meta.get("exposure_time", 0.0))
    readout = float(meta.get("rolling_shutter_time", 0.0))
    s = 1.0 / float(downscale)
    W, H = int(round(meta["w"] * s)), int(round(meta["h"] * s))
    cams, paths, dpaths, npaths = [], [], [], []
    convention = meta.get("normal_convention", "opencv")
    if convention not in NORMAL_CONVENTIONS:
        raise ValueError(f"transforms.json: unknown normal_convention {convention!r} (one of {NORMAL_CONVENTIONS})")
    is_eval_set = set()
    scores = None
    if eval_mode == "blur_score":
        missing = [fr["file_path"] for fr in frames if "motion_blur_score" not in fr]
        if missing:
            raise ValueError(f"eval_mode='blur_score': {len(missing)} frames carry no motion_blur_score (first: "
                             f"{missing[0]}); tools/blur_score.py --write-scores computes them")
        scores = [float(fr["motion_blur_score"]) for fr in frames]
    tr, ev = split_indices([fr["file_path"] for fr in frames], eval_mode, eval_interval, scores)
    is_eval_set.update(ev)
    for i, fr in enumerate(frames):
        c2w = torch.tensor(fr["transform_matrix"], dtype=torch.float32)
        if c2w.shape != (4, 4):
            raise ValueError(f"frame {fr['file_path']}: transform_matrix must be 4x4")
        md = {
            "cam_idx": i,
            "camera_linear_velocity": [float(v) for v in fr.get("camera_linear_velocity", (0.0, 0.0, 0.0))],
            "camera_angular_velocity": [float(v) for v in fr.get("camera_angular_velocity", (0.0, 0.0, 0.0))],
            "exposure_time": exposure,
            "rolling_shutter_time": readout,
            "is_eval": i in is_eval_set and eval_mode != "all",
        }
        if "motion_blur_score" in fr:
            md["motion_blur_score"] = float(fr["motion_blur_score"])
        cams.append(Camera(c2w[:3], float(fr.get("fl_x", meta["fl_x"])) * s, float(fr.get("fl_y", meta["fl_y"])) * s,
                           float(fr.get("cx", meta["cx"])) * s, float(fr.get("cy", meta["cy"])) * s, W, H, md))
        paths.append(os.path.normpath(os.path.join(root, fr["file_path"])))
        dp = fr.get("depth_file_path")
        dpaths.append(os.path.normpath(os.path.join(root, dp)) if dp else None)
        npth = fr.get("normal_file_path")
        npaths.append(os.path.normpath(os.path.join(root, npth)) if npth else None)
    at = meta.get("applied_transform")
    return TransformsScene(
        cameras=cams, image_paths=paths, train_indices=tr, eval_indices=ev, exposure_time=exposure,
        rolling_shutter_time=readout,
        distortion={k: float(meta[k]) for k in ("k1", "k2", "k3", "p1", "p2") if k in meta},
        ply_file_path=(os.path.normpath(os.path.join(root, meta["ply_file_path"])) if "ply_file_path" in meta else None),
        applied_transform=(torch.tensor(at, dtype=torch.float32) if at is not None else None),
        depth_paths=dpaths, depth_unit_scale_factor=float(meta.get("depth_unit_scale_factor", 1e-3)),
        normal_paths=npaths, normal_convention=convention,
    )


def _undistort_grid(H: int, W: int, fx: float, fy: float, cx: float, cy: float, distortion: Dict[str, float], device):
    """source pixel INDEX coordinates (us, vs) [H,W] float64 that the undistorted pixel grid samples"""
    k1, k2, k3 = (float(distortion.get(k, 0.0)) for k in ("k1", "k2", "k3"))
    p1, p2 = float(distortion.get("p1", 0.0)), float(distortion.get("p2", 0.0))
    dt = torch.float64
    v, u = torch.meshgrid(torch.arange(H, device=device, dtype=dt), torch.arange(W, device=device, dtype=dt), indexing="ij")
    # pixel CENTRES at +0.5 (the convention of the rasterizer and of nerfstudio's cameras)
    x, y = (u + 0.5 - cx) / fx, (v + 0.5 - cy) / fy
    r2 = x * x + y * y
    radial = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    xd = x * radial + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    yd = y * radial + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    return xd * fx + cx - 0.5, yd * fy + cy - 0.5


def _has_distortion(distortion: Dict[str, float]) -> bool:
    return any(float(distortion.get(k, 0.0)) != 0.0 for k in ("k1", "k2", "k3", "p1", "p2"))


def undistort_roi(H: int, W: int, fx: float, fy: float, cx: float, cy: float,
                  distortion: Dict[str, float]) -> Tuple[int, int, int, int]:
    """(x0, y0, x1, y1): the largest axis-aligned rectangle of the undistorted frame, grown out from the principal
    point, in which EVERY pixel samples inside the source image.  With pincushion (k1 > 0) or tangential terms the
    border of the undistorted frame looks outside the sensor; nerfstudio's datamanager crops to the valid region
    (cv2.getOptimalNewCameraMatrix(alpha=0) + its ROI) and adopts the new intrinsics, so no black, unmasked pixels reach
    the loss.  Here the focal lengths stay and the frame is cropped: cx, cy shift by (x0, y0)."""
    if not _has_distortion(distortion):
        return 0, 0, W, H
    us, vs = _undistort_grid(H, W, fx, fy, cx, cy, distortion, "cpu")
    ok = (us >= 0.0) & (us <= W - 1.0) & (vs >= 0.0) & (vs <= H - 1.0)      # the bilinear footprint lies inside
    x0, y0, x1, y1 = 0, 0, W, H
    # shrink the side whose border line has the largest share of invalid pixels until all four lines are clean
    while x1 - x0 > 2 and y1 - y0 > 2:
        sides = {"l": (~ok[y0:y1, x0]).float().mean(), "r": (~ok[y0:y1, x1 - 1]).float().mean(),
                 "t": (~ok[y0, x0:x1]).float().mean(), "b": (~ok[y1 - 1, x0:x1]).float().mean()}
        side, bad = max(sides.items(), key=lambda kv: float(kv[1]))
        if float(bad) == 0.0:
            break
        if side == "l":
            x0 += 1
        elif side == "r":
            x1 -= 1
        elif side == "t":
            y0 += 1
        else:
            y1 -= 1
    if not bool(ok[y0:y1, x0:x1].all()):
        raise ValueError("lens distortion leaves no valid rectangle around the principal point")
    return x0, y0, x1, y1


def undistort_image(img: torch.Tensor, fx: float, fy: float, cx: float, cy: float,
                    distortion: Dict[str, float], crop: bool = False):
    """[H,W,3] image taken through OpenCV's radial-tangential lens model (k1, k2, k3, p1, p2 — the fields
    /root/reference/process_synthetic_inputs.py:113-129 and combine.py:109-131 write) -> the image an ideal pinhole
    camera with the SAME focal lengths would see (bilinear).  nerfstudio's datamanager undistorts the training images
    once up front — the rasterizer only knows pinhole cameras.  All-zero coefficients return the input unchanged.
    crop=False: same size and principal point; pixels that look outside the source stay black (no mask!).
    crop=True: -> (image cropped to undistort_roi, (x0, y0, x1, y1)): every pixel valid; the caller shifts cx, cy by
    (x0, y0) and adopts the new size (load_scene_images does)."""
    H, W = img.shape[0], img.shape[1]
    if not _has_distortion(distortion):
        return (img, (0, 0, W, H)) if crop else img
    us, vs = _undistort_grid(H, W, fx, fy, cx, cy, distortion, img.device)
    grid = torch.stack([(us + 0.5) / W * 2.0 - 1.0, (vs + 0.5) / H * 2.0 - 1.0], dim=-1)[None].to(img.dtype)
    out = torch.nn.functional.grid_sample(img.permute(2, 0, 1)[None], grid, mode="bilinear", padding_mode="zeros",
                                          align_corners=False)
    out = out[0].permute(1, 2, 0).contiguous()
    if not crop:
        return out
    x0, y0, x1, y1 = undistort_roi(H, W, fx, fy, cx, cy, distortion)
    return out[y0:y1, x0:x1].contiguous(), (x0, y0, x1, y1)


def load_scene_images(scene: "TransformsScene", device="cpu", undistort: bool = True) -> List[torch.Tensor]:
    """every frame's image, undistorted with the scene's lens coefficients when any is non-zero (what nerfstudio's
    datamanager does before the first iteration).  An undistorted frame is CROPPED to the rectangle in which every pixel
    is valid and `scene.cameras[i]` is replaced by the camera of the cropped frame (cx, cy shifted, new width / height;
    same focal lengths): no black border reaches the loss.  undistort=False returns the frames as stored — cut to the
    cropped cameras' rectangle if an earlier load of this scene object already replaced its cameras."""
    out = []
    lens = undistort and _has_distortion(scene.distortion)
    for i, (cam, path) in enumerate(zip(scene.cameras, scene.image_paths)):
        img = load_image(path, device)
        if lens and not cam.metadata.get("undistorted", False):
            img, (x0, y0, x1, y1) = undistort_image(img, cam.fx, cam.fy, cam.cx, cam.cy, scene.distortion, crop=True)
            md = dict(cam.metadata, undistorted=True, undistort_roi=(x0, y0, x1, y1))
            scene.cameras[i] = Camera(cam.camera_to_world, cam.fx, cam.fy, cam.cx - x0, cam.cy - y0, x1 - x0, y1 - y0, md)
        elif lens:
            # the camera already describes the cropped frame (a second load of the same scene): same crop again
            x0, y0, x1, y1 = cam.metadata["undistort_roi"]
            full = undistort_image(img, cam.fx, cam.fy, cam.cx + x0, cam.cy + y0, scene.distortion)
            img = full[y0:y1, x0:x1].contiguous()
        elif cam.metadata.get("undistorted", False):
            # undistort=False on a scene whose cameras an earlier load already replaced by those of the cropped frames
            # (ADVICE round 4): the raw frame is cut to the same rectangle, so that image size and intrinsics agree —
            # the pixels stay distorted, which is what the caller asked for
            x0, y0, x1, y1 = cam.metadata["undistort_roi"]
            img = img[y0:y1, x0:x1].contiguous()
        out.append(img)
    return out


def load_depth(path: str, scale: float = 1e-3, device="cpu") -> torch.Tensor:
    """[H,W,1] float32 depth in scene units = stored value * scale (nerfstudio's depth_unit_scale_factor: 1e-3 turns
    millimetres into metres), 0 = no measurement (so are non-finite and negative values).  `.npy` (any numeric
    [H,W] or [H,W,1] array) or a single-channel image PIL decodes (16-bit PNG: mode I;16 / I)."""
    import numpy as np
    if path.endswith(".npy"):
        arr = np.load(path)
    else:
        from PIL import Image
        with Image.open(path) as im:
            arr = np.asarray(im)
    arr = np.asarray(arr, dtype=np.float64)
    if arr.ndim == 3:
        arr = arr[..., 0]
    if arr.ndim != 2:
        raise ValueError(f"{path}: a depth map must be [H,W] or [H,W,1], got shape {arr.shape}")
    d = arr * float(scale)
    d[~np.isfinite(d) | (d < 0)] = 0.0
    return torch.from_numpy(d.astype(np.float32))[..., None].to(device)


def undistort_depth(depth: torch.Tensor, fx: float, fy: float, cx: float, cy: float, distortion: Dict[str, float],
                    crop: bool = False):
    """undistort_image for a depth map [H,W,1] with NEAREST-neighbour sampling (an interpolated depth across an edge or
    next to a missing measurement would be a depth nobody measured): pixels that look outside the source, or whose
    nearest source pixel holds no measurement, are 0.  crop=True: cut to the same undistort_roi as the images."""
    H, W = depth.shape[0], depth.shape[1]
    if not _has_distortion(distortion):
        return (depth, (0, 0, W, H)) if crop else depth
    us, vs = _undistort_grid(H, W, fx, fy, cx, cy, distortion, depth.device)
    ui, vi = torch.round(us).long(), torch.round(vs).long()
    inside = (ui >= 0) & (ui < W) & (vi >= 0) & (vi < H)
    src = depth[..., 0]
    out = torch.where(inside, src[vi.clamp(0, H - 1), ui.clamp(0, W - 1)], torch.zeros((), dtype=depth.dtype))[..., None]
    out = out.to(depth.dtype).contiguous()
    if not crop:
        return out
    x0, y0, x1, y1 = undistort_roi(H, W, fx, fy, cx, cy, distortion)
    return out[y0:y1, x0:x1].contiguous(), (x0, y0, x1, y1)


def load_scene_depths(scene: "TransformsScene", device="cpu", undistort: bool = True) -> List[Optional[torch.Tensor]]:
    """every frame's depth map [H,W,1] (load_depth with the scene's depth_unit_scale_factor), or None for a frame
    without one — undistorted (nearest neighbour) and cropped exactly like load_scene_images' frames, whether or not
    that call has already replaced scene.cameras by the cropped cameras."""
    out: List[Optional[torch.Tensor]] = []
    lens = undistort and _has_distortion(scene.distortion)
    paths = scene.depth_paths or [None] * len(scene.cameras)
    for cam, path in zip(scene.cameras, paths):
        if path is None:
            out.append(None)
            continue
        d = load_depth(path, scene.depth_unit_scale_factor, device)
        if cam.metadata.get("undistorted", False):
            # the camera describes the cropped frame: undistort with the full frame's principal point, same rectangle
            x0, y0, x1, y1 = cam.metadata["undistort_roi"]
            full = undistort_depth(d, cam.fx, cam.fy, cam.cx + x0, cam.cy + y0, scene.distortion) if lens else d
            d = full[y0:y1, x0:x1].contiguous()
        elif lens:
            d, _ = undistort_depth(d, cam.fx, cam.fy, cam.cx, cam.cy, scene.distortion, crop=True)
        out.append(d)
    return out


def _read_png_rgb16(path: str):
    """a non-interlaced 16-bit RGB(A) PNG -> uint16 [H,W,3], or None for any other file (PIL reads those; it would cut a
    16-bit colour PNG to 8 bits).  Rows filtered with Average or Paeth are undone pixel by pixel in Python: slow, exact"""
    import struct
    import zlib
    import numpy as np
    with open(path, "rb") as f:
        raw = f.read()
    if raw[:8] != b"\x89PNG\r\n\x1a\n":
        return None
    pos, idat, head = 8, [], None
    while pos + 8 <= len(raw):
        n, kind = struct.unpack(">I4s", raw[pos:pos + 8])
        body = raw[pos + 8:pos + 8 + n]
        pos += 12 + n
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            break
    if head is None or head[2] != 16 or head[3] not in (2, 6) or head[6] != 0:
        return None
    W, H, C = head[0], head[1], 3 if head[3] == 2 else 4
    bpp, stride = 2 * C, 2 * C * W
    data = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8).reshape(H, stride + 1)
    out = np.zeros((H + 1, stride), np.uint8)
    for y in range(H):
        ft, row, up = int(data[y, 0]), data[y, 1:].astype(np.int64), out[y].astype(np.int64)
        if ft == 0:
            cur = row
        elif ft == 2:
            cur = row + up
        elif ft == 1:
            cur = np.cumsum(row.reshape(W, bpp), axis=0).reshape(-1)
        elif ft in (3, 4):
            cur = np.zeros(stride, np.int64)
            for i in range(stride):
                a = int(cur[i - bpp]) if i >= bpp else 0
                b = int(up[i])
                c = int(up[i - bpp]) if i >= bpp else 0
                if ft == 3:
                    pred = (a + b) // 2
                else:
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                cur[i] = (int(row[i]) + pred) & 255
        else:
            raise ValueError(f"{path}: PNG filter type {ft}")
        out[y + 1] = (cur & 255).astype(np.uint8)
    px = out[1:].reshape(H, W, C, 2).astype(np.uint16)
    return (px[..., 0] << 8 | px[..., 1])[..., :3]


def load_normal(path: str, convention: str = "opencv", device="cpu") -> torch.Tensor:
    """[H,W,3] float32 normal map in the camera frame of normals.depth_normals (x right, y down, z forward).  `.npy`: a
    float [H,W,3] array of vectors; an 8- or 16-bit RGB PNG: n = 2 v / max - 1 per channel.  convention "opengl" (x right, y
    up, z towards the viewer): y and z are negated.  Vectors are not normalised here (the op does it); a non-finite vector
    becomes the zero vector, "no value"."""
    import numpy as np
    if convention not in NORMAL_CONVENTIONS:
        raise ValueError(f"unknown normal_convention {convention!r} (one of {NORMAL_CONVENTIONS})")
    if path.endswith(".npy"):
        arr = np.asarray(np.load(path), dtype=np.float64)
    else:
        px = _read_png_rgb16(path)
        if px is None:
            from PIL import Image
            with Image.open(path) as im:
                px = np.asarray(im.convert("RGB"))
        arr = 2.0 * px.astype(np.float64) / float(np.iinfo(px.dtype).max) - 1.0
    if arr.ndim != 3 or arr.shape[-1] != 3:
        raise ValueError(f"{path}: a normal map must be [H,W,3], got shape {arr.shape}")
    arr = arr.copy()
    arr[~np.isfinite(arr).all(-1)] = 0.0
    if convention == "opengl":
        arr[..., 1:] *= -1.0
    return torch.from_numpy(arr.astype(np.float32)).to(device)


def undistort_normals(normals: torch.Tensor, fx: float, fy: float, cx: float, cy: float, distortion: Dict[str, float],
                      crop: bool = False):
    """undistort_depth for a normal map [H,W,3]: NEAREST-neighbour sampling, zero vectors for pixels that look outside the
    source.  The vectors themselves are kept: the small rotation a lens undistortion implies for a direction is ignored."""
    H, W = normals.shape[0], normals.shape[1]
    if not _has_distortion(distortion):
        return (normals, (0, 0, W, H)) if crop else normals
    us, vs = _undistort_grid(H, W, fx, fy, cx, cy, distortion, normals.device)
    ui, vi = torch.round(us).long(), torch.round(vs).long()
    inside = (ui >= 0) & (ui < W) & (vi >= 0) & (vi < H)
    out = torch.where(inside[..., None], normals[vi.clamp(0, H - 1), ui.clamp(0, W - 1)], torch.zeros((), dtype=normals.dtype))
    out = out.to(normals.dtype).contiguous()
    if not crop:
        return out
    x0, y0, x1, y1 = undistort_roi(H, W, fx, fy, cx, cy, distortion)
    return out[y0:y1, x0:x1].contiguous(), (x0, y0, x1, y1)


def load_scene_normals(scene: "TransformsScene", device="cpu", undistort: bool = True) -> List[Optional[torch.Tensor]]:
    """every frame's normal prior [H,W,3] (load_normal with the scene's normal_convention), or None for a frame without
    one — undistorted (nearest neighbour; the directions are not rotated, see undistort_normals) and cropped exactly like
    load_scene_depths' maps."""
    out: List[Optional[torch.Tensor]] = []
    lens = undistort and _has_distortion(scene.distortion)
    paths = scene.normal_paths or [None] * len(scene.cameras)
    for cam, path in zip(scene.cameras, paths):
        if path is None:
            out.append(None)
            continue
        n = load_normal(path, scene.normal_convention, device)
        if cam.metadata.get("undistorted", False):
            x0, y0, x1, y1 = cam.metadata["undistort_roi"]
            full = undistort_normals(n, cam.fx, cam.fy, cam.cx + x0, cam.cy + y0, scene.distortion) if lens else n
            n = full[y0:y1, x0:x1].contiguous()
        elif lens:
            n, _ = undistort_normals(n, cam.fx, cam.fy, cam.cx, cam.cy, scene.distortion, crop=True)
        out.append(n)
    return out


def load_image(path: str, device="cpu") -> torch.Tensor:
    """[H,W,3] float32 in 0..1.  `.npy` (float, already 0..1) or anything PIL decodes (8-bit PNG / JPEG)."""
    if path.endswith(".npy"):
        import numpy as np
        return torch.from_numpy(np.load(path).astype("float32"))[..., :3].to(device)
    import numpy as np
    from PIL import Image
    with Image.open(path) as im:
        arr = np.asarray(im.convert("RGB"), dtype=np.uint8)
    return (torch.from_numpy(arr.copy()).to(device).float() / 255.0)


def save_image(path: str, img: torch.Tensor) -> None:
    """[H,W,3] float 0..1 -> 8-bit PNG (or .npy float32 when the name says so)"""
    import numpy as np
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    a = img.detach().clamp(0, 1).cpu()
    if path.endswith(".npy"):
        np.save(path, a.numpy().astype("float32"))
        return
    from PIL import Image
    Image.fromarray((a * 255.0 + 0.5).to(torch.uint8).numpy()).save(path)


def write_transforms(root: str, width: int, height: int, fx: float, fy: float, cx: float, cy: float,
                     exposure_time: float, rolling_shutter_time: float, frames: List[Dict],
                     ply_file_path: Optional[str] = None) -> str:
    """Write transforms.json with exactly the fields of /root/reference/process_synthetic_inputs.py:113-129 (top
    level) and :171-176 (per frame: camera_linear_velocity, camera_angular_velocity, file_path, transform_matrix)."""
    meta = {"aabb_scale": 16, "cx": float(cx), "cy": float(cy), "exposure_time": float(exposure_time),
            "fl_x": float(fx), "fl_y": float(fy), "frames": [], "h": int(height), "k1": 0, "k2": 0,
            "orientation_override": "none", "p1": 0, "p2": 0, "rolling_shutter_time": float(rolling_shutter_time),
            "w": int(width)}
    for fr in frames:
        meta["frames"].append({
            "camera_angular_velocity": [float(v) for v in fr["camera_angular_velocity"]],
            "camera_linear_velocity": [float(v) for v in fr["camera_linear_velocity"]],
            "file_path": fr["file_path"],
            "transform_matrix": [[float(v) for v in row] for row in fr["transform_matrix"]]})
    if ply_file_path is not None:
        meta["ply_file_path"] = ply_file_path
    os.makedirs(root, exist_ok=True)
    out = os.path.join(root, "transforms.json")
    with open(out, "wt") as f:
        json.dump(meta, f, indent=4)
    return out


def write_seed_points_ply(path: str, xyz: torch.Tensor, rgb: torch.Tensor, binary: bool = False) -> None:
    """ASCII PLY `x y z red green blue` like /root/reference/process_synthetic_inputs.py:203-219; binary: the same columns
    as binary_little_endian 1.0 (what COLMAP, Open3D and MeshLab write), the coordinates as full float32"""
    n = xyz.shape[0]
    if binary:
        import numpy as np
        rows = np.zeros(n, dtype=np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"),
                                           ("blue", "u1")]))
        c = (rgb.clamp(0, 1) * 255.0 + 0.5).to(torch.int64).clamp(max=255).numpy()
        for j, name in enumerate(("x", "y", "z")):
            rows[name] = xyz[:, j].detach().cpu().float().numpy()
        for j, name in enumerate(("red", "green", "blue")):
            rows[name] = c[:, j]
        header = "\n".join(["ply", "format binary_little_endian 1.0", f"element vertex {n}", "property float x",
                            "property float y", "property float z", "property uchar red", "property uchar green",
                            "property uchar blue", "end_header"]) + "\n"
        with open(path, "wb") as f:
            f.write(header.encode("ascii"))
            f.write(rows.tobytes())
        return
    lines = ["ply", "format ascii 1.0", f"element vertex {n}", "property float x", "property float y",
             "property float z", "property uint8 red", "property uint8 green", "property uint8 blue", "end_header"]
    c = (rgb.clamp(0, 1) * 255.0 + 0.5).to(torch.int64)
    for i in range(n):
        lines.append(f"{xyz[i, 0].item():.6f} {xyz[i, 1].item():.6f} {xyz[i, 2].item():.6f} "
                     f"{int(c[i, 0])} {int(c[i, 1])} {int(c[i, 2])}")
    with open(path, "wt") as f:
        f.write("\n".join(lines) + "\n")


def _load_seed_points_binary(raw: bytes, header_end: int, header: List[str]) -> Tuple[torch.Tensor, torch.Tensor]:
    """the vertex element of a binary_little_endian PLY: columns found by name, other scalar columns skipped"""
    import numpy as np
    from .checkpoint import _PLY_TYPES
    n, fields, element = None, [], None
    for ln in header[1:]:
        t = ln.split()
        if not t or t[0] in ("comment", "obj_info"):
            continue
        if t[0] == "element":
            if len(t) != 3:
                raise ValueError(f"malformed PLY header line {ln!r}")
            if n is None and t[1] != "vertex":
                raise ValueError(f"PLY element {t[1]!r} stands before the vertex element")
            element = t[1]
            if element == "vertex":
                n = int(t[2])
        elif t[0] == "property" and element == "vertex":
            if len(t) != 3 or t[1] not in _PLY_TYPES:
                raise ValueError(f"vertex property {ln!r}: only scalar properties of the standard PLY types are read")
            fields.append((t[2], "<" + _PLY_TYPES[t[1]]))
    if n is None:
        raise ValueError("PLY without a vertex element")
    names = [nm for nm, _ in fields]
    if len(set(names)) != len(names):
        raise ValueError("PLY with a repeated vertex property name")
    missing = [p for p in ("x", "y", "z") if p not in names]
    if missing:
        raise ValueError(f"PLY seed cloud misses the properties {missing}")
    dtype = np.dtype(fields)
    body = raw[header_end:]
    if len(body) < n * dtype.itemsize:
        raise ValueError(f"truncated PLY body: {len(body)} bytes for {n} rows of {dtype.itemsize}")
    rows = np.frombuffer(body, dtype=dtype, count=n)

    def take(cols):
        return torch.from_numpy(np.stack([rows[c].astype(np.float32) for c in cols], axis=1)).reshape(n, 3)
    has_rgb = all(c in names for c in ("red", "green", "blue"))
    rgb = take(["red", "green", "blue"]) / 255.0 if has_rgb else torch.full((n, 3), 0.5)
    return take(["x", "y", "z"]), rgb


def load_seed_points_ply(path: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """PLY seed cloud `x y z red green blue` -> (xyz [N,3] float32, rgb [N,3] float32 in 0..1): ASCII
    (/root/reference/process_synthetic_inputs.py:203-219) or binary_little_endian 1.0 (COLMAP, Open3D, MeshLab), where the
    columns are found by name, other scalar columns are skipped and a list property of the vertex element is a
    ValueError."""
    import re
    with open(path, "rb") as f:
        raw = f.read()
    m = re.search(rb"end_header[ \t]*\r?\n", raw)
    if raw.startswith(b"ply") and m is not None:
        header = raw[:m.start()].decode("ascii", errors="replace").splitlines()
        fmt = next((ln.split()[1:] for ln in header if ln.split()[:1] == ["format"]), None)
        if fmt and fmt[0] == "binary_little_endian":
            return _load_seed_points_binary(raw, m.end(), header)
        if fmt and fmt[0] != "ascii":
            raise ValueError(f"PLY format {fmt[0]!r}: seed clouds are read as ascii or binary_little_endian")
    with open(path, "rt") as f:
        lines = f.read().splitlines()
    if not lines or lines[0].strip() != "ply":
        raise ValueError("not a PLY file")
    n, props, i = 0, [], 0
    for i, ln in enumerate(lines):
        t = ln.split()
        if t[:2] == ["element", "vertex"]:
            n = int(t[2])
        elif t[:1] == ["property"]:
            props.append(t[-1])
        elif t[:1] == ["format"] and t[1] != "ascii":
            raise ValueError("only ASCII PLY seed clouds are supported")
        elif t[:1] == ["end_header"]:
            break
    rows = [[float(v) for v in ln.split()] for ln in lines[i + 1:i + 1 + n]]
    data = torch.tensor(rows, dtype=torch.float32).reshape(n, len(props))
    col = {p: j for j, p in enumerate(props)}
    xyz = data[:, [col["x"], col["y"], col["z"]]]
    rgb = data[:, [col["red"], col["green"], col["blue"]]] / 255.0 if "red" in col else torch.full((n, 3), 0.5)
    return xyz, rgb


def velocities_from_poses(c2ws, times=None, loop: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """Finite-difference camera-frame velocities of a pose sequence, for datasets that carry poses only: the rule of
    /root/reference/render_video.py:85-115.  c2ws [F,3 or 4,4] camera-to-world; -> (linear [F,3], angular [F,3]) float64,
    each in the axes of its own frame's camera (the axes c2ws uses, so OpenGL poses give what transforms.json stores).
    Frame i is differenced between its neighbours i - 1 and i + 1 — clamped to the ends of an open path, so the ends are
    one-sided, and taken modulo F when loop is set: world-frame translation difference and the rotation vector (SO(3)
    log) of R_next R_prev^T, both divided by delta_t and rotated into frame i.  delta_t = times[next] - times[prev];
    times=None counts in frame indices, delta_t = next - prev as the reference has it (across the wrap of a looped path
    that is 2 - F, not 2: the reference's own convention, kept).  A single frame has zero velocity."""
    c2ws = torch.as_tensor(c2ws, dtype=torch.float64)
    if c2ws.dim() != 3 or c2ws.shape[1] not in (3, 4) or c2ws.shape[2] != 4:
        raise ValueError(f"c2ws must be [F,3,4] or [F,4,4], got {tuple(c2ws.shape)}")
    F = int(c2ws.shape[0])
    idx = torch.arange(F)
    prev, nxt = ((idx - 1) % F, (idx + 1) % F) if loop else ((idx - 1).clamp(min=0), (idx + 1).clamp(max=F - 1))
    t = idx.to(torch.float64) if times is None else torch.as_tensor(times, dtype=torch.float64).reshape(F)
    dt = t[nxt] - t[prev]
    if F > 1 and bool((dt == 0).any()):
        raise ValueError("two neighbouring frames share a time stamp")
    dt = torch.where(dt == 0, torch.ones_like(dt), dt)                  # F == 1: both differences are zero anyway
    R, p = c2ws[:, :3, :3], c2ws[:, :3, 3]
    lin_w = (p[nxt] - p[prev]) / dt[:, None]
    ang_w = _so3_log(R[nxt] @ R[prev].transpose(1, 2)) / dt[:, None]
    R_wc = R.transpose(1, 2)
    return (R_wc @ lin_w[:, :, None])[:, :, 0], (R_wc @ ang_w[:, :, None])[:, :, 0]


def _so3_log(R: torch.Tensor) -> torch.Tensor:
    """rotation vectors [...,3] of rotation matrices [...,3,3] (float64), angle in [0, pi]: the angle from atan2 of the
    antisymmetric part's norm and the trace, the axis from the antisymmetric part — or, within 1e-6 of pi where that
    vanishes, from the largest column of R + I"""
    a = torch.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], dim=-1)
    s = a.norm(dim=-1)                                                   # 2 sin(angle)
    c = R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1.0                 # 2 cos(angle)
    angle = torch.atan2(s, c)
    small = s < 1e-12
    scale = torch.where(small, torch.full_like(s, 0.5), angle / torch.where(small, torch.ones_like(s), s))
    out = a * scale[..., None]
    flipped = (s < 2e-6) & (c < 0)                                       # angle ~ pi: a carries no direction
    if bool(flipped.any()):
        S = R + torch.eye(3, dtype=R.dtype, device=R.device)             # = 2 n n^T at angle pi
        k = torch.diagonal(S, dim1=-2, dim2=-1).argmax(dim=-1)
        n = torch.gather(S, -1, k[..., None, None].expand(S.shape[:-1] + (1,)))[..., 0]
        n = n / n.norm(dim=-1, keepdim=True)
        sign = torch.where((n * a).sum(-1) < 0, -1.0, 1.0)
        out = torch.where(flipped[..., None], n * (sign * angle)[..., None], out)
    return out


def camera_arrays(cameras) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """what blur_stats takes, from the cameras' poses and metadata alone: (viewmats [F,4,4], lin [F,3], ang [F,3], intrins
    [F,4], times [F,2]) float32 on the CPU, poses and velocities through blurscore.view_and_twist"""
    from .blurscore import view_and_twist
    c2w = torch.stack([c.camera_to_world[:3].to(dtype=torch.float32, device="cpu") for c in cameras])
    vel = [torch.tensor([[float(v) for v in c.metadata.get(k, (0.0, 0.0, 0.0))] for c in cameras], dtype=torch.float32)
           for k in ("camera_linear_velocity", "camera_angular_velocity")]
    viewmats, lin, ang = view_and_twist(c2w, vel[0], vel[1])
    intrins = torch.tensor([[c.fx, c.fy, c.cx, c.cy] for c in cameras], dtype=torch.float32)
    times = torch.tensor([[float(c.metadata.get("exposure_time", 0.0)), float(c.metadata.get("rolling_shutter_time", 0.0))]
                          for c in cameras], dtype=torch.float32)
    return viewmats, lin, ang, intrins, times


def blur_stats(scene: "TransformsScene", points: torch.Tensor):
    """blurscore.BlurStats of every frame of `scene` (in its camera order) over `points` [N,3] — the seed cloud, say — from
    the dataset's own poses, velocities and times, no model: on points' device (a GPU cloud takes the HIP kernels)."""
    from .blurscore import blur_stats as _stats
    cams = scene.cameras
    if not cams:
        raise ValueError("the scene has no frames")
    if any((c.width, c.height) != (cams[0].width, cams[0].height) for c in cams):
        raise ValueError("blur_stats needs frames of one size")
    points = points.detach().to(torch.float32)
    arrays = (t.to(points.device) for t in camera_arrays(cams))
    return _stats(points, *arrays, cams[0].width, cams[0].height)


def blur_scores(scene: "TransformsScene", points: torch.Tensor) -> List[float]:
    """one motion_blur_score per frame of `scene`: the mean streak length in pixels (blur_stats(...).mean_blur)"""
    return [float(v) for v in blur_stats(scene, points).mean_blur.tolist()]


def write_blur_scored(src_root: str, dst_root: str, scores=None, interval: int = 8) -> str:
    """Write the blur-scored copy of the dataset at src_root to dst_root, as
    /root/reference/train_eval_split_by_blur_score.py:6-57 does: frames sorted by file_path and cut into runs of `interval`,
    the frame with the smallest score of each run copied to images/eval_<name>, the others to images/train_<name>,
    file_path rewritten to the copy, every other key of transforms.json kept, sparse_pc.ply copied when there is one.
    scores: one per frame in path-sorted order (the order of load_transforms' cameras), stored as motion_blur_score; None
    uses the scores the file holds (ValueError when a frame has none).  An image is looked up at src_root/<file_path>.
    load_transforms(dst_root, eval_mode="filename") then reads the split.  -> the path of the written transforms.json"""
    import shutil
    if os.path.abspath(src_root) == os.path.abspath(dst_root):
        raise ValueError("write_blur_scored writes a copy: dst_root must differ from src_root")
    with open(os.path.join(src_root, "transforms.json"), "rt") as f:
        meta = json.load(f)
    frames = meta["frames"] = sorted(meta["frames"], key=lambda fr: fr["file_path"])
    if scores is not None:
        if len(scores) != len(frames):
            raise ValueError(f"{len(scores)} scores for {len(frames)} frames")
        for fr, sc in zip(frames, scores):
            fr["motion_blur_score"] = float(sc)
    paths = [fr["file_path"] for fr in frames]
    if any("motion_blur_score" not in fr for fr in frames):
        raise ValueError("a frame carries no motion_blur_score and no scores were given")
    _, ev = split_indices(paths, "blur_score", interval, [fr["motion_blur_score"] for fr in frames])
    os.makedirs(os.path.join(dst_root, "images"), exist_ok=True)
    chosen = set(ev)
    for i, fr in enumerate(frames):
        name = ("eval_" if i in chosen else "train_") + os.path.basename(paths[i])
        shutil.copyfile(os.path.join(src_root, paths[i]), os.path.join(dst_root, "images", name))
        fr["file_path"] = os.path.join("images", name)
    ply = os.path.join(src_root, "sparse_pc.ply")
    if os.path.exists(ply):
        shutil.copyfile(ply, os.path.join(dst_root, "sparse_pc.ply"))
    out = os.path.join(dst_root, "transforms.json")
    with open(out, "wt") as f:
        json.dump(meta, f, indent=4)
    return out


def synthetic_scene(n: int, width: int, height: int, sh_degree: int = 3, seed: int = 1234,
                    scale_mult: float = 1.0, profile: str = "survey") -> Dict:
    """The seeded benchmark scene of SURVEY.md §8d (the inputs bench.py measures on): camera at the origin,
    OpenCV axes, fx = fy = 0.8*W; Gaussians uniform in the frustum slab z in [1,10] reaching 1.2x the field
    of view, log-scales ~ N(log(0.004 * 5.5 * scale_mult), 0.6^2), random unit quaternions, opacity logits
    ~ N(0, 2^2), SH dc ~ N(0, 0.5^2), higher bands ~ N(0, 0.05^2); camera velocity 0.1*U[-1,1]^3 m/s and
    0.2*U[-1,1]^3 rad/s, exposure 1/60 s, readout 1/30 s.  Raw (pre-activation) float32 parameters on the CPU.
    The test oracle draws the same scene from the same generator sequence (tests/test_host_logic.py pins it).
    profile="trained" keeps every random draw but shapes the scene like a fitted model instead of SURVEY §8d's
    saturated one: world-space scale proportional to depth (0.006 * z: every Gaussian is ~7 px wide on screen,
    none fills the view) and mostly translucent opacities (logits ~ N(-3.3, 1.5^2)) — pixels need hundreds of
    list entries before they saturate, a large share of the Gaussians receives a gradient and the depth-sliced
    path needs several slices (bench.py reports it as config.secondary)."""
    import math
    g = torch.Generator().manual_seed(seed)
    fx = fy = 0.8 * width
    z = 1.0 + 9.0 * torch.rand(n, generator=g)
    u = (torch.rand(n, generator=g) * 2 - 1) * 1.2
    v = (torch.rand(n, generator=g) * 2 - 1) * 1.2
    means = torch.stack([u * z * (0.5 * width / fx), v * z * (0.5 * height / fy), z], -1)
    log_scales = math.log(0.004 * 5.5 * scale_mult) + 0.6 * torch.randn(n, 3, generator=g)
    quats = torch.randn(n, 4, generator=g)
    quats = quats / quats.norm(dim=-1, keepdim=True)
    opacity_logits = 2.0 * torch.randn(n, generator=g)
    if profile == "trained":
        log_scales = log_scales - math.log(0.004 * 5.5) + torch.log(0.006 * z)[:, None]
        opacity_logits = opacity_logits * 0.75 - 3.3
    elif profile != "survey":
        raise ValueError(f"unknown scene profile {profile!r}")
    K = (sh_degree + 1) ** 2
    sh = torch.cat([0.5 * torch.randn(n, 1, 3, generator=g), 0.05 * torch.randn(n, K - 1, 3, generator=g)], 1)
    lin_vel = 0.1 * (torch.rand(3, generator=g) * 2 - 1)
    ang_vel = 0.2 * (torch.rand(3, generator=g) * 2 - 1)
    return dict(means=means, log_scales=log_scales, quats=quats, opacity_logits=opacity_logits, sh=sh,
                viewmat=torch.eye(4), lin_vel=lin_vel, ang_vel=ang_vel, fx=fx, fy=fy, cx=width / 2.0,
                cy=height / 2.0, exposure_time=1.0 / 60.0, rolling_shutter_time=1.0 / 30.0)
