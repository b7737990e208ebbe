"""Splatfacto-style model surface over the HIP hot path.

Mirrors what the reference needs from the nerfstudio fork's ``SplatfactoModel``
(absent submodule, /root/reference/.gitmodules:1-3):
  * config fields set by /root/reference/train.py:14-22,40,46-70,119-120
    (rasterize_mode, blur_samples, rolling_shutter_compensation, gamma, min_rgb_level,
    camera_optimizer.mode, camera_velocity_optimizer.*, background_color, ...)
  * ``get_outputs_for_camera(camera=...)`` returning ``rgb`` and ``depth`` and honouring
    ``camera.metadata['cam_idx']``                      (/root/reference/render_model.py:216-219)
  * per-frame ``camera_linear_velocity`` / ``camera_angular_velocity`` in the (OpenGL) camera
    frame plus scene-level ``exposure_time`` / ``rolling_shutter_time``
    (/root/reference/process_synthetic_inputs.py:113-129,157-176).
The forward/backward rendering surface; the densification step that follows it lives in densify.py
(SURVEY §8 f3); the trainer, data managers and the viewer are out of scope.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch
from torch import Tensor, nn

from . import ops


@dataclass
class CameraOptimizerConfig:
    mode: str = "off"  # "off" | "SO3xR3"   (train.py:40)


@dataclass
class CameraVelocityOptimizerConfig:
    enabled: bool = False                 # train.py:66
    zero_initial_velocities: bool = False  # train.py:70


SH_C0 = 0.28209479177387814           # the SH band-0 basis value: colour = 0.5 + SH_C0 * sh[0]
SHUTTER_EXPOSURE_MODES = ("off", "global", "per_camera")
SHUTTER_READOUT_MODES = ("off", "global")


@dataclass
class CameraShutterOptimizerConfig:
    """learnable exposure / rolling-shutter readout times: log-scale adjustments, zero at the start, on the
    camera's metadata values — E = E0 * exp(adj), T = T0 * exp(adj).  SE(3) motion model only."""
    exposure: str = "off"                  # "off" | "global" (one adjustment) | "per_camera" (one per cam_idx)
    readout: str = "off"                   # "off" | "global"
    # starting values for cameras whose metadata holds 0 / nothing, used ONLY for a quantity that is being optimised
    # (a zero time has no gradient direction in a log parametrisation: metadata 0 and no fallback is a ValueError)
    initial_exposure_time: Optional[float] = None
    initial_rolling_shutter_time: Optional[float] = None


@dataclass
class SplatfactoDeblurConfig:
    sh_degree: int = 3
    sh_degree_interval: int = 0              # splatfacto raises the active SH degree every 1000 steps; 0 = all bands at once
    rasterize_mode: str = "antialiased"      # train.py:119 ("classic" disables the compensation factor)
    use_scale_regularization: bool = False   # train.py:120 (loss-side; carried for CLI parity)
    blur_samples: int = 5                    # train.py:46,51 ; 0 disables motion-blur sampling
    rolling_shutter_compensation: bool = True  # train.py:56
    rs_bands: int = 10                       # row bands per frame when rolling-shutter compensation is on
    gamma: float = 2.2                       # train.py:62 (gamma=1 when gamma correction is off)
    min_rgb_level: float = 0.0               # train.py:60 (10 with gamma correction)
    background_color: str = "black"          # train.py:17 ("auto" = learnable)
    num_downscales: int = 0                  # train.py:14; splatfacto's default is 2: training starts at 1/2^n resolution
    resolution_schedule: int = 3000          # ... and doubles every this many steps (nerfstudio 1.1.0 default)
    cull_scale_thresh: float = 0.5           # train.py:18 (densification; carried for CLI parity)
    optimize_eval_velocities: bool = True    # train.py:20
    output_depth_during_training: bool = False
    # how a sub-pose moves the splats: "se3" re-projects every Gaussian under the screw-interpolated pose
    # (north_star), "pixel_velocity" is the paper's first-order model — one projection, centres shifted by
    # t * pixel velocity, depth order / covariance / colour of the mid-exposure pose
    motion_model: str = "se3"
    # rolling shutter (with rolling_shutter_compensation): "bands" = rs_bands tile-row bands, each its own sub-pose
    # (both motion models); "exact" (pixel_velocity only) = continuous per-row time inside the compositor, ONE
    # projection / sort per blur sample whatever the band count (SURVEY App. A "row time (y/H - 1/2) * T_ro")
    rolling_shutter_mode: str = "bands"
    # pixel_velocity only: "per_sample" = one projection / sort / tile list per sub-pose; "shared" = ONE for the frame
    # (tile boxes swept over the exposure + readout, every blur sample walks the same list — the form the paper
    # describes; rolling shutter then only in its "exact" mode)
    pixel_velocity_lists: str = "per_sample"
    camera_optimizer: CameraOptimizerConfig = field(default_factory=CameraOptimizerConfig)
    camera_velocity_optimizer: CameraVelocityOptimizerConfig = field(default_factory=CameraVelocityOptimizerConfig)
    # learnable exposure / readout times; "off"/"off": no parameter, no optimizer, the host schedule as it always was
    camera_shutter_optimizer: CameraShutterOptimizerConfig = field(default_factory=CameraShutterOptimizerConfig)
    # "adam": every Gaussian row steps every iteration (torch.optim.Adam); "selective_adam": only the rows the step's
    # views reached (gsplat's SelectiveAdam) — the others keep parameter and both moments unchanged
    optimizer: str = "adam"
    # selective_adam's row mask: "visible" = radii > 0 in any sub-pose of any camera of the step (gsplat's rule);
    # "touched" = any non-zero gradient in any Gaussian parameter (what the compositor reached)
    selective_mask: str = "visible"
    # densification statistic: True = training renders also fill model.xy_absgrad, the per-(pixel, Gaussian) absolute
    # centre gradient summed over pixels and sub-poses (ops.render_subposes xy_absgrad_out; densify.DensifyConfig.absgrad
    # reads it).  SE(3) motion model only: the pixel-velocity model refuses it (ValueError)
    densify_absgrad: bool = False
    # 3DGS-MCMC's regularisers (mcmc.py relies on them to let Gaussians die; upstream 0.01 each): the loss gains
    # opacity_reg * mean(sigmoid(opacities)) + scale_reg * mean(exp(scales)).  0.0: the step is unchanged, nothing is built
    opacity_reg: float = 0.0
    scale_reg: float = 0.0
    # per-image bilateral-grid colour correction (bilagrid.py; gsplat's lib_bilagrid / splatfacto's use_bilateral_grid):
    # training renders of a camera that names itself (metadata['cam_idx']) pass through that camera's learned lattice of
    # affine colour transforms before the loss; evaluation renders never do.  False: no parameter, no optimizer, no launch
    use_bilateral_grid: bool = False
    grid_shape: Tuple[int, int, int] = (16, 16, 8)     # (GW, GH, L)
    bilateral_grid_tv_lambda: float = 10.0             # weight of the total-variation penalty on all grids
    # evaluation only (splatfacto's name): train_step.evaluate also reports cc_psnr / cc_ssim, taken after each render was
    # fitted to its ground truth by a per-channel quadratic colour warp (colorcorrect.py).  False: same keys, same path
    color_corrected_metrics: bool = False


@dataclass
class Camera:
    """Minimal stand-in for nerfstudio's Cameras (one camera).  camera_to_world uses the dataset's
    OpenGL convention (-z forward, +y up; process_synthetic_inputs.py:230-238)."""
    camera_to_world: Tensor  # [3,4] or [4,4]
    fx: float
    fy: float
    cx: float
    cy: float
    width: int
    height: int
    metadata: Dict = field(default_factory=dict)  # cam_idx, camera_linear_velocity, camera_angular_velocity,
    #                                               exposure_time, rolling_shutter_time

    def rescaled(self, d: int) -> "Camera":
        """the same camera at 1/d of the resolution (nerfstudio's rescale_output_resolution(1/d), floor rounding):
        what splatfacto renders while its resolution schedule is active"""
        s = 1.0 / float(d)
        return Camera(self.camera_to_world, self.fx * s, self.fy * s, self.cx * s, self.cy * s,
                      int(self.width * s), int(self.height * s), self.metadata)


def _skew(w: Tensor) -> Tensor:
    z = torch.zeros((), device=w.device, dtype=w.dtype)
    return torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])


def _so3_exp(w: Tensor) -> Tensor:
    th2 = (w * w).sum()
    K = _skew(w)
    eye = torch.eye(3, device=w.device, dtype=w.dtype)
    small = th2 < 1e-10
    th = torch.sqrt(torch.clamp(th2, min=1e-20))
    A = torch.where(small, 1.0 - th2 / 6.0, torch.sin(th) / th)
    B = torch.where(small, 0.5 - th2 / 24.0, (1.0 - torch.cos(th)) / torch.clamp(th2, min=1e-20))
    return eye + A * K + B * (K @ K)


def expected_depth(depth_acc: Tensor, alphas: Tensor) -> Tensor:
    """splatfacto's outputs["depth"] from the compositor's per-sample depth sums depth_acc [S,H,W] (sum of weight *
    camera-space depth) and alphas [S,H,W]: d / a with d, a their means over the samples, [H,W,1].  Differentiable in d
    and a; zero-alpha pixels hold far = d.max(), detached — splatfacto 1.1.0 fills them with depth_im.detach().max(), the
    UN-normalised accumulated maximum (what render_model.py:219's colour maps are normalised against)."""
    d = depth_acc.mean(dim=0)[..., None]
    a = alphas.mean(dim=0)[..., None]
    far = d.detach().max()
    return torch.where(a > 0, d / torch.clamp(a, min=1e-10), far)


class SplatfactoDeblurModel(nn.Module):
    """Gaussian parameters + ``get_outputs`` through the fused HIP path."""

    _sharp = False          # set by sharp_outputs for the length of one render: exposure and readout count as 0

    def __init__(self, config: SplatfactoDeblurConfig, means: Tensor, log_scales: Tensor, quats: Tensor,
                 opacity_logits: Tensor, features_dc: Tensor, features_rest: Tensor, num_cameras: int = 1):
        super().__init__()
        self.config = config
        # parameter names follow splatfacto's gauss_params
        self.means = nn.Parameter(means.float())
        self.scales = nn.Parameter(log_scales.float())
        self.quats = nn.Parameter(quats.float())
        self.opacities = nn.Parameter(opacity_logits.float().reshape(-1, 1))
        self.features_dc = nn.Parameter(features_dc.float())
        self.features_rest = nn.Parameter(features_rest.float())
        if config.background_color == "auto":
            self.background_param = nn.Parameter(torch.zeros(3))
        else:
            self.background_param = None
        self.num_cameras = num_cameras
        if config.camera_optimizer.mode == "SO3xR3":
            self.pose_adjustment = nn.Parameter(torch.zeros(num_cameras, 6))
        elif config.camera_optimizer.mode == "off":
            self.pose_adjustment = None
        else:
            raise ValueError(f"unknown camera_optimizer.mode {config.camera_optimizer.mode!r}")
        if config.camera_velocity_optimizer.enabled:
            self.velocity_adjustment = nn.Parameter(torch.zeros(num_cameras, 6))
        else:
            self.velocity_adjustment = None
        sh = config.camera_shutter_optimizer
        if sh.exposure not in SHUTTER_EXPOSURE_MODES:
            raise ValueError(f"unknown camera_shutter_optimizer.exposure {sh.exposure!r} (one of {SHUTTER_EXPOSURE_MODES})")
        if sh.readout not in SHUTTER_READOUT_MODES:
            raise ValueError(f"unknown camera_shutter_optimizer.readout {sh.readout!r} (one of {SHUTTER_READOUT_MODES})")
        if (sh.exposure != "off" or sh.readout != "off") and config.motion_model == "pixel_velocity":
            raise ValueError("camera_shutter_optimizer needs motion_model='se3': the pixel-velocity model takes the "
                             "sub-pose times inside its projection and compositors, which return no time gradient")
        # log-scale adjustments, zero at the start: "per_camera" rows are indexed by metadata['cam_idx']
        self.exposure_adjustment = (None if sh.exposure == "off" else
                                    nn.Parameter(torch.zeros(num_cameras if sh.exposure == "per_camera" else 1)))
        self.readout_adjustment = None if sh.readout == "off" else nn.Parameter(torch.zeros(1))
        if config.use_bilateral_grid:
            from . import bilagrid
            self.bilateral_grids = nn.Parameter(bilagrid.identity_grids(num_cameras, config.grid_shape))
        else:
            self.bilateral_grids = None
        self.step = 0                        # training iteration (advanced by train_step)
        self.radii: Optional[Tensor] = None
        # densification statistics (densify.py): when enabled, every training render leaves the summed
        # screen-space centre gradient of its backward pass in self.xy_grad [N,2] (pixels)
        self.collect_densify_stats = False
        self.xy_grad: Optional[Tensor] = None
        # config.densify_absgrad: the absgrad statistic of the same render, same shape(s) as xy_grad
        self.xy_absgrad: Optional[Tensor] = None
        self._group_xy_absgrad: Optional[Tensor] = None
        self.last_size = (0, 0)
        # frame-to-frame memory of THIS model's frames (adaptive slice budget, arena estimate): owned here, not by the
        # binding's module state, so two models of one shape never share it
        self.frame_hints = ops.FrameHints()

    def _hints_of(self, camera):
        """a camera that names itself (metadata['cam_idx'], as the datamanager's training cameras do:
        /root/reference/render_model.py:216-219) has its own memory inside this model's FrameHints (ops.FrameHints.view): a
        training loop revisits the same cameras, and what a frame teaches the next one is a property of the camera; a
        camera without an index (a novel view) goes through the scene-level memory"""
        idx = camera.metadata.get("cam_idx") if camera.metadata else None
        return self.frame_hints if idx is None else self.frame_hints.view(int(idx))

    # -- splatfacto-style accessors ------------------------------------------------
    @property
    def num_points(self) -> int:
        return self.means.shape[0]

    def active_sh_degree(self) -> int:
        """splatfacto's progressive SH schedule: degree min(step // sh_degree_interval, sh_degree) while training"""
        cfg = self.config
        if not self.training or cfg.sh_degree_interval <= 0:
            return cfg.sh_degree
        return min(self.step // cfg.sh_degree_interval, cfg.sh_degree)

    def gauss_params(self) -> Dict[str, nn.Parameter]:
        return {"means": self.means, "scales": self.scales, "quats": self.quats, "opacities": self.opacities,
                "features_dc": self.features_dc, "features_rest": self.features_rest}

    def _background(self, device) -> Tensor:
        c = self.config.background_color
        if c == "auto":
            return torch.sigmoid(self.background_param).to(device)
        if c == "random" and self.training:
            return torch.rand(3, device=device)
        if c == "white":
            return torch.ones(3, device=device)
        return torch.zeros(3, device=device)

    # -- camera handling -------------------------------------------------------------
    def _const(self, values) -> Tensor:
        """small constant on the parameters' device, uploaded once (a fresh torch.tensor(list, device=...) is a
        pageable host->device copy, i.e. a stream synchronisation, every frame)"""
        key = (tuple(float(v) for v in values), str(self.means.device))
        cache = self.__dict__.setdefault("_const_cache", {})
        t = cache.get(key)
        if t is None:
            if len(cache) > 256:
                cache.clear()
            t = cache[key] = torch.tensor(key[0], dtype=torch.float32, device=self.means.device)
        return t

    def _camera_inputs(self, camera: Camera):
        """the camera's pose and data velocities on the parameters' device, uploaded ONCE per camera: a pageable
        host->device copy of a 48-byte tensor is ordered behind everything queued on the stream, i.e. it blocks the host
        until the previous iteration's kernels have drained — three of them per frame cost a training loop its whole
        host run-ahead (round 5; the cache lives on the Camera object and follows its tensors' identity / values)"""
        dev = self.means.device
        md = camera.metadata
        lin_h = tuple(float(v) for v in md.get("camera_linear_velocity", (0.0, 0.0, 0.0)))
        ang_h = tuple(float(v) for v in md.get("camera_angular_velocity", (0.0, 0.0, 0.0)))
        key = (str(dev), id(camera.camera_to_world), camera.camera_to_world._version, lin_h, ang_h)
        hit = camera.__dict__.get("_gsd_device_inputs")
        if hit is None or hit[0] != key:
            c2w = camera.camera_to_world.to(device=dev, dtype=torch.float32)
            hit = (key, c2w, torch.tensor(lin_h, dtype=torch.float32, device=dev),
                   torch.tensor(ang_h, dtype=torch.float32, device=dev))
            camera.__dict__["_gsd_device_inputs"] = hit
        return hit[1], hit[2], hit[3]

    def _viewmat_and_velocity(self, camera: Camera):
        dev = self.means.device
        c2w, lin_data, ang_data = self._camera_inputs(camera)
        static = self.pose_adjustment is None and self.velocity_adjustment is None
        if static:
            # no camera-side parameters: (viewmat, lin, ang) is a pure function of the camera — a dozen tiny launches
            # per frame otherwise
            tag = (camera.__dict__["_gsd_device_inputs"][0], bool(self.config.camera_velocity_optimizer.zero_initial_velocities))
            hit = camera.__dict__.get("_gsd_view")
            if hit is not None and hit[0] == tag:
                return hit[1]
        R_gl, t = c2w[:3, :3], c2w[:3, 3]
        cam_idx = int(camera.metadata.get("cam_idx", 0))
        if self.pose_adjustment is not None and 0 <= cam_idx < self.num_cameras:
            # nerfstudio's camera optimizer composes in the CAMERA frame: c2w @ exp_map_SO3xR3(adj)
            adj = self.pose_adjustment[cam_idx]
            t = t + R_gl @ adj[:3]
            R_gl = R_gl @ _so3_exp(adj[3:])
        flip = self._const([1.0, -1.0, -1.0])
        R_cv = R_gl * flip[None, :]                # OpenGL -> OpenCV camera axes (x, -y, -z)
        R_wc = R_cv.T
        t_wc = -(R_wc @ t)
        viewmat = torch.eye(4, device=dev)
        viewmat = torch.cat([torch.cat([R_wc, t_wc[:, None]], dim=1), viewmat[3:4]], dim=0)
        md = camera.metadata
        zero3 = self._const([0.0, 0.0, 0.0])
        use_data_vel = not self.config.camera_velocity_optimizer.zero_initial_velocities
        lin, ang = lin_data, ang_data
        if not use_data_vel:
            lin, ang = zero3, zero3
        # velocities are given in the OpenGL camera frame (process_synthetic_inputs.py:163-165)
        lin, ang = lin * flip, ang * flip
        if self.velocity_adjustment is not None and 0 <= cam_idx < self.num_cameras:
            is_eval = bool(md.get("is_eval", False))
            adj = self.velocity_adjustment[cam_idx]
            if is_eval and not self.config.optimize_eval_velocities:
                adj = adj.detach() * 0.0
            lin, ang = lin + adj[:3], ang + adj[3:]
        if static:
            camera.__dict__["_gsd_view"] = (tag, (viewmat, lin, ang))
        return viewmat, lin, ang

    def _schedule(self, camera: Camera):
        cfg = self.config
        S = cfg.blur_samples if cfg.blur_samples > 0 else 1
        R = cfg.rs_bands if cfg.rolling_shutter_compensation else 1
        # (with the shutter optimizer: the effective STARTING values, fallbacks included, decide S = 1 / R = 1)
        exposure, readout = self._base_times(camera)
        if exposure == 0.0:
            S = 1
        if readout == 0.0:
            R = 1
        if cfg.rolling_shutter_mode == "exact":
            if cfg.motion_model != "pixel_velocity":
                raise ValueError("rolling_shutter_mode='exact' needs motion_model='pixel_velocity'")
            R = 1                                   # the row time lives in the compositor (see _rs_time)
        elif cfg.rolling_shutter_mode != "bands":
            raise ValueError(f"unknown rolling_shutter_mode {cfg.rolling_shutter_mode!r}")
        if cfg.pixel_velocity_lists == "shared":
            if cfg.motion_model != "pixel_velocity" or R != 1:
                raise ValueError("pixel_velocity_lists='shared' needs motion_model='pixel_velocity' and, with a rolling "
                                 "shutter, rolling_shutter_mode='exact'")
        elif cfg.pixel_velocity_lists != "per_sample":
            raise ValueError(f"unknown pixel_velocity_lists {cfg.pixel_velocity_lists!r}")
        times, _, _ = ops.subpose_schedule(S, exposure, R, readout)
        return S, R, times

    def _base_times(self, camera: Camera) -> Tuple[float, float]:
        """(E0, T0): the camera's metadata exposure / rolling-shutter time; for a quantity the shutter optimizer learns, a
        metadata value of 0 (or none) is replaced by camera_shutter_optimizer.initial_*, and 0 there too is a ValueError.
        Inside sharp_outputs both are 0: one sample at the camera's effective pose."""
        if self._sharp:
            return 0.0, 0.0
        exposure = float(camera.metadata.get("exposure_time", 0.0))
        readout = float(camera.metadata.get("rolling_shutter_time", 0.0))
        sh = self.config.camera_shutter_optimizer
        if self.exposure_adjustment is not None and exposure == 0.0:
            exposure = float(sh.initial_exposure_time or 0.0)
            if exposure == 0.0:
                raise ValueError("camera_shutter_optimizer.exposure is on, the camera's exposure_time is 0 / absent and "
                                 "initial_exposure_time gives no start: E = E0 * exp(adj) cannot leave 0")
        if self.readout_adjustment is not None and readout == 0.0:
            readout = float(sh.initial_rolling_shutter_time or 0.0)
            if readout == 0.0:
                raise ValueError("camera_shutter_optimizer.readout is on, the camera's rolling_shutter_time is 0 / absent "
                                 "and initial_rolling_shutter_time gives no start: T = T0 * exp(adj) cannot leave 0")
        return exposure, readout

    def shutter_times(self, camera: Camera) -> Tuple[Tensor, Tensor]:
        """the effective (exposure, readout) of `camera` as 0-d tensors on the parameters' device: E0 * exp(adjustment)
        for a learned quantity (differentiable), the base value otherwise.  A "per_camera" exposure adjustment applies
        to cam_idx inside [0, num_cameras); a camera without one renders with E0."""
        E0, T0 = self._base_times(camera)
        E, T = self._const([E0]).reshape(()), self._const([T0]).reshape(())
        if self.exposure_adjustment is not None:
            if self.config.camera_shutter_optimizer.exposure == "per_camera":
                idx = camera.metadata.get("cam_idx") if camera.metadata else None
                if idx is not None and 0 <= int(idx) < int(self.exposure_adjustment.shape[0]):
                    E = E * torch.exp(self.exposure_adjustment[int(idx)])
            else:
                E = E * torch.exp(self.exposure_adjustment[0])
        if self.readout_adjustment is not None:
            T = T * torch.exp(self.readout_adjustment[0])
        return E, T

    def _times_tensor(self, camera: Camera, S: int, R: int, times) -> Tensor:
        """the sub-pose times on the device: the cached host schedule, or — shutter optimizer on — ops.subpose_times of
        the learned exposure / readout (differentiable)"""
        if self.exposure_adjustment is None and self.readout_adjustment is None:
            return self._const(times)
        E, T = self.shutter_times(camera)
        return ops.subpose_times(S, E, R, T, device=self.means.device)

    def _rs_time(self, camera: Camera) -> float:
        """readout time handed to the exact rolling-shutter compositors (0: off)"""
        cfg = self.config
        if cfg.rolling_shutter_mode != "exact" or not cfg.rolling_shutter_compensation or self._sharp:
            return 0.0
        return float(camera.metadata.get("rolling_shutter_time", 0.0))

    # -- rendering ---------------------------------------------------------------------
    # -- bilateral grid ----------------------------------------------------------------
    def _grid_index(self, camera: Camera, bilateral_grid: Optional[bool]) -> Optional[int]:
        """the index of the bilateral grid a render of `camera` passes through, or None.  bilateral_grid None: apply iff
        the model has grids, is training and the camera names itself; True / False force it.  Raises ValueError — before
        any launch — when the grid is asked for and absent, or cam_idx is outside [0, num_cameras)."""
        idx = camera.metadata.get("cam_idx") if camera.metadata else None
        if bilateral_grid is None:
            bilateral_grid = self.bilateral_grids is not None and self.training and idx is not None
        if not bilateral_grid:
            return None
        if self.bilateral_grids is None:
            raise ValueError("bilateral_grid=True needs a model built with SplatfactoDeblurConfig.use_bilateral_grid")
        if idx is None:
            raise ValueError("bilateral_grid=True needs camera.metadata['cam_idx']")
        idx = int(idx)
        if not 0 <= idx < int(self.bilateral_grids.shape[0]):
            raise ValueError(f"cam_idx {idx} outside [0, {int(self.bilateral_grids.shape[0])}): no bilateral grid for it")
        return idx

    def get_outputs(self, camera: Camera, detach_gaussians: bool = False,
                    return_depth: Optional[bool] = None, bilateral_grid: Optional[bool] = None) -> Dict[str, Tensor]:
        """_render's outputs; with the bilateral grid (bilateral_grid None: iff config.use_bilateral_grid, self.training
        and 'cam_idx' in the camera's metadata) out["rgb"] is the colour-corrected image bilagrid.slice(grids, rgb,
        cam_idx).  get_outputs_for_camera never corrects."""
        gi = self._grid_index(camera, bilateral_grid)
        out = self._render(camera, detach_gaussians, return_depth)
        if gi is not None:
            from . import bilagrid
            out["rgb"] = bilagrid.slice(self.bilateral_grids, out["rgb"], gi)
        return out

    def _render(self, camera: Camera, detach_gaussians: bool = False,
                return_depth: Optional[bool] = None) -> Dict[str, Tensor]:
        """detach_gaussians=True renders with the Gaussians as constants: only the camera-side parameters (pose /
        velocity adjustment, background) receive a gradient — what the fork's `--optimize-eval-cameras`
        (/root/reference/train.py:180-183, README.md:197) needs for the evaluation frames.
        out["depth"] (rendered with output_depth_during_training, in eval, or with return_depth=True) is differentiable
        in training: a depth loss reaches the Gaussians and the camera adjustments (expected_depth)."""
        cfg = self.config
        dev = self.means.device
        d = self.downscale_factor()
        if d > 1:
            camera = camera.rescaled(d)          # splatfacto: camera.rescale_output_resolution(1 / d) while training
        viewmat, lin, ang = self._viewmat_and_velocity(camera)
        S, R, times = self._schedule(camera)
        times_t = self._times_tensor(camera, S, R, times)
        pixvel = cfg.motion_model == "pixel_velocity"
        if not pixvel and cfg.motion_model != "se3":
            raise ValueError(f"unknown motion_model {cfg.motion_model!r}")
        viewmats = viewmat if pixvel else ops.subpose_viewmats(viewmat, lin, ang, times_t)
        shared = pixvel and cfg.pixel_velocity_lists == "shared"
        # the RAW parameters go to the kernels as they are: log-scales, opacity logits, features_dc / features_rest as two
        # pointers (no exp / sigmoid / cat launches and none of their backward; ops.render_combined raw_params / sh_rest)
        gp = (self.means, self.scales, self.quats, self.opacities, self.features_dc, self.features_rest)
        if detach_gaussians:
            gp = tuple(t.detach() for t in gp)
        means_, scales_, quats_, opac_, dc_, rest_ = gp
        bg = self._background(dev)
        use_gamma = cfg.blur_samples > 0
        self.xy_grad = self.xy_absgrad = None
        if self.training and self.collect_densify_stats and not detach_gaussians:
            self.xy_grad = torch.zeros(self.num_points, 2, device=dev)
            if cfg.densify_absgrad:
                self.xy_absgrad = torch.zeros(self.num_points, 2, device=dev)
        gamma = cfg.gamma if use_gamma else 1.0
        min_level = cfg.min_rgb_level if use_gamma else 0.0
        # one autograd node for composite + gamma-space average: no [S,H,W,3] sample-gradient tensor in backward
        want_depth = (cfg.output_depth_during_training or not self.training) if return_depth is None else bool(return_depth)
        res = ops.render_combined(
            means_, scales_, quats_, opac_.reshape(-1), dc_,
            viewmats, bg, S, R, camera.fx, camera.fy, camera.cx, camera.cy, camera.height, camera.width,
            gamma=gamma, min_rgb_level=min_level, sh_degree=self.active_sh_degree(),
            antialiased=(cfg.rasterize_mode == "antialiased"), xy_grad_out=self.xy_grad,
            lin_vel=lin if pixvel else None, ang_vel=ang if pixvel else None,
            times=(list(times) if shared else times_t) if pixvel else None,
            return_depth=want_depth, rolling_shutter_time=self._rs_time(camera) if pixvel else 0.0,
            sh_rest=rest_, raw_params=True, shared_list=shared, hints=self._hints_of(camera),
            xy_absgrad_out=self.xy_absgrad)
        rgb, alphas, radii = res[:3]
        depth_acc = res[3] if want_depth else None
        self.radii = radii
        self.last_size = (camera.width, camera.height)
        accumulation = alphas.mean(dim=0)[..., None]
        out = {"rgb": torch.clamp(rgb, max=1.0),      # splatfacto clamps in training too
               "accumulation": accumulation, "background": bg}
        if depth_acc is not None:
            out["depth"] = expected_depth(depth_acc, alphas)
        else:
            out["depth"] = None
        return out

    def render_and_backward(self, camera: Camera, grad_image, grad_depth=None, grad_depth_sums=None) -> Tensor:
        """One TRAINING frame, forward and backward in one host call (step.render_step: the same C-ABI calls as
        get_outputs + Tensor.backward, without the autograd engine between the two compositors — the entry bench.py
        times).  grad_image: callable rgb [H,W,3] -> d loss / d rgb, where rgb is what get_outputs()["rgb"] would hold
        (clamped at 1).  Gradients ACCUMULATE into .grad of the Gaussian parameters; pose / velocity adjustments and a
        learnable background get theirs through the small torch graph of _viewmat_and_velocity / _background.
        Returns rgb (detached).  Same values as the autograd route (tests: test_train_step_routes_agree).
        grad_depth (optional): callable (depth [H,W,1], accumulation [H,W,1]) -> d loss / d depth [H,W,1], where depth is
        what get_outputs()["depth"] would hold (expected_depth); its chain to the per-sample depth sums and alphas runs
        here, and the frame's backward takes the depth term (step.render_step grad_depth).  None: rgb and every gradient
        exactly as without it.
        grad_depth_sums (optional, instead of grad_depth: both is a ValueError): callable (depth_acc [S,H,W], alphas
        [S,H,W]) -> (d loss / d depth_acc, d loss / d alphas), handed to step.render_step(grad_depth=) as it is — a loss
        that starts from the compositor's raw sums (depthprior.depth_prior_loss_with_grad) builds no expected_depth graph."""
        from .step import render_step
        if grad_depth is not None and grad_depth_sums is not None:
            raise ValueError("render_and_backward takes grad_depth or grad_depth_sums, not both")
        cfg = self.config
        dev = self.means.device
        d = self.downscale_factor()
        if d > 1:
            camera = camera.rescaled(d)
        viewmat, lin, ang = self._viewmat_and_velocity(camera)
        S, R, times = self._schedule(camera)
        pixvel = cfg.motion_model == "pixel_velocity"
        if not pixvel and cfg.motion_model != "se3":
            raise ValueError(f"unknown motion_model {cfg.motion_model!r}")
        shared = pixvel and cfg.pixel_velocity_lists == "shared"
        bg = self._background(dev)
        use_gamma = cfg.blur_samples > 0
        self.xy_grad = self.xy_absgrad = None
        if self.training and self.collect_densify_stats:
            self.xy_grad = torch.zeros(self.num_points, 2, device=dev)
            if cfg.densify_absgrad:
                self.xy_absgrad = torch.zeros(self.num_points, 2, device=dev)
        cam_leaves = [t for t in (viewmat, lin, ang) if t.requires_grad]
        times_t = None if shared else self._times_tensor(camera, S, R, times)
        times_grad = times_t is not None and times_t.requires_grad      # (the shutter optimizer: SE(3) only)

        def v_rgb(rgb):
            # get_outputs clamps rgb at 1 before the loss sees it; the clamp's backward is the mask
            v = grad_image(torch.clamp(rgb, max=1.0))
            return v * (rgb <= 1.0)

        v_depth = grad_depth_sums
        if grad_depth is not None:
            def v_depth(depth_acc, alphas):
                da, al = depth_acc.requires_grad_(True), alphas.requires_grad_(True)
                depth = expected_depth(da, al)
                v = grad_depth(depth.detach(), al.detach().mean(dim=0)[..., None])
                if v is None:
                    raise ValueError("grad_depth(depth, accumulation) returned None: it must return d loss / d depth")
                return torch.autograd.grad(depth, (da, al), v.detach().reshape(depth.shape), allow_unused=True)

        rgb, g, radii = render_step(
            self.means, self.scales, self.quats, self.opacities.reshape(-1), self.features_dc, viewmat.detach(),
            lin.detach(), ang.detach(), list(times) if shared else (times_t.detach() if times_grad else times_t), bg.detach(), S, R,
            camera.fx, camera.fy, camera.cx, camera.cy, camera.height, camera.width, v_rgb,
            gamma=cfg.gamma if use_gamma else 1.0, min_rgb_level=cfg.min_rgb_level if use_gamma else 0.0,
            sh_degree=self.active_sh_degree(), antialiased=(cfg.rasterize_mode == "antialiased"),
            sh_rest=self.features_rest, raw_params=True, motion_model=cfg.motion_model, xy_grad_out=self.xy_grad,
            camera_grads=bool(cam_leaves), background_grad=bg.requires_grad,
            rolling_shutter_time=self._rs_time(camera) if pixvel else 0.0, shared_list=shared, hints=self._hints_of(camera),
            grad_depth=v_depth, xy_absgrad_out=self.xy_absgrad, **({"times_grad": True} if times_grad else {}))
        for p, gr in ((self.means, g["means"]), (self.scales, g["scales"]), (self.quats, g["quats"]),
                      (self.opacities, g["opacities"]), (self.features_dc, g["sh"]), (self.features_rest, g["sh_rest"])):
            gr = gr.view_as(p)
            p.grad = gr if p.grad is None else p.grad + gr
        roots, seeds = [], []
        for t, key in ((viewmat, "viewmat"), (lin, "lin_vel"), (ang, "ang_vel")):
            if t.requires_grad and g[key] is not None:
                roots.append(t)
                seeds.append(g[key].view_as(t))
        if bg.requires_grad and g["background"] is not None:
            roots.append(bg)
            seeds.append(g["background"].view_as(bg))
        if times_grad and g["times"] is not None:
            # d loss / d times [P] into the graph of ops.subpose_times: exposure / readout adjustments
            roots.append(times_t)
            seeds.append(g["times"].view_as(times_t))
        if roots:
            torch.autograd.backward(roots, seeds)
        self.radii = radii
        self.last_size = (camera.width, camera.height)
        return torch.clamp(rgb, max=1.0)

    def downscale_factor(self) -> int:
        """splatfacto's `_get_downscale_factor` (nerfstudio 1.1.0): while training, render (and compare) at
        1 / 2^max(num_downscales - step // resolution_schedule, 0) of the camera's resolution; full size otherwise
        (/root/reference/train.py:14 sets num-downscales 0 for the low-resolution synthetic sets)."""
        if not self.training:
            return 1
        return 2 ** max(int(self.config.num_downscales) - int(self.step) // max(1, int(self.config.resolution_schedule)), 0)

    def _batch_groups(self, cameras):
        """(rescaled camera, S, R, times) per camera, grouped by what one frame must share — fx, fy, cx, cy, H, W, S,
        R — in the order of each group's first camera: [(key, [input positions])]"""
        d = self.downscale_factor()
        items, groups = [], {}
        for j, cam in enumerate(cameras):
            if d > 1:
                cam = cam.rescaled(d)          # each camera follows the resolution schedule, as in get_outputs
            S, R, times = self._schedule(cam)
            items.append((cam, S, R, times))
            key = (float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy), int(cam.height), int(cam.width), S, R)
            groups.setdefault(key, []).append(j)
        return items, list(groups.items())

    def _render_group(self, items, return_depth: bool, detach_gaussians: bool = False):
        """ONE ops.render_batch frame for cameras that share intrinsics, size, S and R: each camera keeps its own pose
        and velocity adjustments (by cam_idx), exposure and rolling-shutter schedule"""
        cfg = self.config
        dev = self.means.device
        cam0, S, R, _ = items[0]
        vms = []
        for cam, _, _, times in items:
            viewmat, lin, ang = self._viewmat_and_velocity(cam)
            vms.append(ops.subpose_viewmats(viewmat, lin, ang, self._times_tensor(cam, S, R, times)))
        viewmats = torch.stack(vms)
        gp = (self.means, self.scales, self.quats, self.opacities, self.features_dc, self.features_rest)
        if detach_gaussians:
            gp = tuple(t.detach() for t in gp)
        means_, scales_, quats_, opac_, dc_, rest_ = gp
        bg = self._background(dev)
        use_gamma = cfg.blur_samples > 0
        xy = xy_abs = None
        if self.training and self.collect_densify_stats and not detach_gaussians:
            xy = torch.zeros(len(items), self.num_points, 2, device=dev)
            if cfg.densify_absgrad:
                xy_abs = torch.zeros(len(items), self.num_points, 2, device=dev)
        idx = [c.metadata.get("cam_idx") if c.metadata else None for c, _, _, _ in items]
        hints = self.frame_hints if any(i is None for i in idx) else self.frame_hints.view(("batch",) + tuple(int(i) for i in idx))
        res = ops.render_batch(
            means_, scales_, quats_, opac_.reshape(-1), dc_, viewmats, bg, S, R, cam0.fx, cam0.fy, cam0.cx, cam0.cy,
            cam0.height, cam0.width, gamma=cfg.gamma if use_gamma else 1.0,
            min_rgb_level=cfg.min_rgb_level if use_gamma else 0.0, sh_degree=self.active_sh_degree(),
            antialiased=(cfg.rasterize_mode == "antialiased"), return_depth=return_depth, sh_rest=rest_,
            raw_params=True, xy_grad_out=xy, hints=hints, xy_absgrad_out=xy_abs)
        self._group_xy_absgrad = xy_abs          # (beside the return value, whose shape callers and tests rely on)
        return res, xy, bg

    def get_outputs_batch(self, cameras, detach_gaussians: bool = False,
                          return_depth: Optional[bool] = None, bilateral_grid: Optional[bool] = None) -> Dict:
        """_render_batch's outputs; bilateral_grid as in get_outputs, decided per camera: the corrected cameras pass
        through their grids in ONE bilagrid.slice call when the batch is one tensor, one call each otherwise."""
        cameras = list(cameras)
        gis = [self._grid_index(c, bilateral_grid) for c in cameras]
        out = self._render_batch(cameras, detach_gaussians, return_depth)
        if any(g is not None for g in gis):
            from . import bilagrid
            rgb = out["rgb"]
            if isinstance(rgb, Tensor) and all(g is not None for g in gis):
                out["rgb"] = bilagrid.slice(self.bilateral_grids, rgb, gis)
            else:
                out["rgb"] = [r if g is None else bilagrid.slice(self.bilateral_grids, r, g) for r, g in zip(rgb, gis)]
                if isinstance(rgb, Tensor):
                    out["rgb"] = torch.stack(out["rgb"])
        return out

    def _render_batch(self, cameras, detach_gaussians: bool = False,
                      return_depth: Optional[bool] = None) -> Dict:
        """get_outputs for a list of cameras through ops.render_batch: one frame per group of cameras that share
        intrinsics, size, blur samples and row bands (groups in the order of their first camera; outputs in input
        order).  -> {"rgb" [B,H,W,3], "depth" [B,H,W,1] or None, "accumulation" [B,H,W,1], "background"}; when the
        cameras' sizes differ, "rgb" / "depth" / "accumulation" are lists of per-camera tensors instead.
        Training keeps self.radii [B,S*R,N] and self.xy_grad [B,N,2] per camera (lists of per-camera tensors for
        several groups), and self.xy_absgrad likewise with config.densify_absgrad.  SE(3) motion model only."""
        cfg = self.config
        if cfg.motion_model != "se3":
            raise NotImplementedError("get_outputs_batch renders the SE(3) motion model; the pixel-velocity model renders "
                                      "one camera per call (get_outputs)")
        cameras = list(cameras)
        if not cameras:
            raise ValueError("get_outputs_batch needs at least one camera")
        want_depth = (cfg.output_depth_during_training or not self.training) if return_depth is None else bool(return_depth)
        items, groups = self._batch_groups(cameras)
        rgb, acc, depth, radii, xys, xas = ([None] * len(cameras) for _ in range(6))
        bg = None
        for _, pos in groups:
            self._group_xy_absgrad = None
            (g_rgb, g_alphas, g_radii, *g_depth), g_xy, bg = self._render_group([items[j] for j in pos], want_depth,
                                                                                detach_gaussians)
            g_xa = self._group_xy_absgrad
            g_acc = g_alphas.mean(dim=1)[..., None]
            g_dep = [expected_depth(g_depth[0][k], g_alphas[k]) for k in range(len(pos))] if want_depth else None
            for k, j in enumerate(pos):
                rgb[j], acc[j], radii[j] = torch.clamp(g_rgb[k], max=1.0), g_acc[k], g_radii[k]
                depth[j] = g_dep[k] if g_dep is not None else None
                xys[j] = g_xy[k] if g_xy is not None else None
                xas[j] = g_xa[k] if g_xa is not None else None
        same = len({tuple(r.shape) for r in rgb}) == 1
        if len(groups) == 1:
            # one frame: the batch's own tensors (its backward writes the xy_grad rows)
            self.radii, self.xy_grad, self.xy_absgrad = g_radii, g_xy, g_xa
        else:
            self.radii, self.xy_grad = radii, (None if xys[0] is None else xys)
            self.xy_absgrad = None if xas[0] is None else xas
        self.last_size = (items[0][0].width, items[0][0].height)
        out = {"background": bg}
        if same:
            out["rgb"], out["accumulation"] = torch.stack(rgb), torch.stack(acc)
            out["depth"] = torch.stack(depth) if want_depth else None
        else:
            out["rgb"], out["accumulation"], out["depth"] = rgb, acc, (depth if want_depth else None)
        return out

    @torch.no_grad()
    def get_outputs_for_cameras(self, cameras) -> Dict:
        """no_grad eval form of get_outputs_batch (the batched get_outputs_for_camera)"""
        was = self.training
        self.eval()
        try:
            return self.get_outputs_batch(cameras)      # eval mode: never colour-corrected
        finally:
            self.train(was)

    @torch.no_grad()
    def get_outputs_for_camera(self, camera: Camera) -> Dict[str, Tensor]:
        """Eval entry point used by /root/reference/render_model.py:217."""
        was = self.training
        self.eval()
        try:
            return self.get_outputs(camera)             # eval mode: never colour-corrected
        finally:
            self.train(was)

    @torch.no_grad()
    def sharp_outputs(self, camera: Camera) -> Dict[str, Tensor]:
        """get_outputs_for_camera with exposure and readout 0: one sample at the camera's effective pose (pose adjustment
        included, cam_idx kept), whatever the metadata and the shutter optimizer hold — the render without motion blur."""
        was = self.training
        self.eval()
        self._sharp = True
        try:
            return self.get_outputs(camera)
        finally:
            self._sharp = False
            self.train(was)

    @torch.no_grad()
    def fuse_tsdf(self, cameras, volume=None, resolution: int = 256, bounds=None, trunc: Optional[float] = None,
                  min_alpha: float = 0.5, depth_max: Optional[float] = None, sharp: bool = True, batch: Optional[int] = None):
        """Fuse the rendered depth (and colour) of `cameras` into a tsdf.TSDFVolume and return it (tsdf.py: the rule;
        gs.tsdf_extract_mesh turns it into a mesh).  No gradient, eval mode, so the bilateral grid is never applied.
        sharp: render every camera with sharp_outputs (fusing blurred depth would smear the surface); otherwise as
        get_outputs_for_camera.  Pixels with accumulation >= min_alpha have weight 1, the rest 0.
        volume None: a new one over `bounds` = (lo [3], hi [3]) — None: the box of the means between the 2nd and the 98th
        percentile per axis, padded by 5 % of its size on every side — with cubic voxels sized so that the longest axis has
        `resolution` samples.  trunc None: 4 voxels.  depth_max None: no far cut-off.  batch (None: tsdf.FRAMES_PER_LAUNCH)
        views go into one tsdf_integrate call; cameras of another image size start a new call."""
        from . import tsdf as T
        cameras = list(cameras)
        dev = self.means.device
        if volume is None:
            if bounds is None:
                srt = self.means.detach().float().sort(dim=0).values
                n = int(srt.shape[0])
                lo, hi = srt[int(0.02 * (n - 1))], srt[int(math.ceil(0.98 * (n - 1)))]
                pad = 0.05 * (hi - lo)
                lo, hi = lo - pad, hi + pad
            else:
                lo, hi = (torch.as_tensor(b, dtype=torch.float32).reshape(3) for b in bounds)
            lo, hi = [float(v) for v in lo.tolist()], [float(v) for v in hi.tolist()]
            size = [h - l for l, h in zip(lo, hi)]
            if int(resolution) < T.MIN_DIM or not all(math.isfinite(v) and v >= 0 for v in size) or max(size) <= 0:
                raise ValueError(f"fuse_tsdf needs resolution >= {T.MIN_DIM} and a box of positive size, got {resolution}, {lo}, {hi}")
            voxel = max(size) / (int(resolution) - 1)
            dims = [min(T.MAX_DIM, max(T.MIN_DIM, int(math.ceil(v / voxel - 1e-6)) + 1)) for v in size]
            volume = T.TSDFVolume(lo, voxel, dims, device=dev, color=True)
        trunc = 4.0 * volume.voxel_size if trunc is None else float(trunc)
        batch = T.FRAMES_PER_LAUNCH if batch is None else max(1, int(batch))
        far = math.inf if depth_max is None else float(depth_max)
        pending = []                                  # (depth [H,W], colour [H,W,3], weights [H,W], viewmat, intrin)

        def flush():
            if pending:
                d, c, w, v, k = (torch.stack(col) for col in zip(*pending))
                T.tsdf_integrate(volume, d, v, k, trunc, color=c if volume.color is not None else None, weights=w,
                                 depth_max=far)
                pending.clear()
        for camera in cameras:
            out = self.sharp_outputs(camera) if sharp else self.get_outputs_for_camera(camera)
            if out.get("depth") is None:
                raise ValueError("fuse_tsdf needs a render with depth")
            depth = out["depth"].detach().float()
            depth = depth[..., 0] if depth.dim() == 3 else depth
            if pending and pending[0][0].shape != depth.shape:
                flush()
            viewmat = self._viewmat_and_velocity(camera)[0].detach().float()
            acc = out["accumulation"].detach().float().reshape(depth.shape)
            intrin = torch.tensor([camera.fx, camera.fy, camera.cx, camera.cy], dtype=torch.float32).to(dev)
            pending.append((depth.contiguous(), out["rgb"].detach().float().clamp(0.0, 1.0), (acc >= float(min_alpha)).float(),
                            viewmat, intrin))
            if len(pending) >= batch:
                flush()
        flush()
        return volume

    @torch.no_grad()
    def render_normals(self, camera: Camera, sharp: bool = True, min_alpha: float = 0.5) -> Tensor:
        """[H,W,3] normals of the rendered depth of `camera` (normals.depth_normals: camera-frame unit vectors, x right, y
        down, z forward, facing the camera; zeros where a pixel or one of its four neighbours has accumulation <=
        min_alpha).  sharp: render with sharp_outputs, otherwise as get_outputs_for_camera.  No gradient, eval mode."""
        from .normals import depth_normals
        out = self.sharp_outputs(camera) if sharp else self.get_outputs_for_camera(camera)
        if out.get("depth") is None:
            raise ValueError("render_normals needs a render with depth")
        H, W = int(camera.height), int(camera.width)
        depth = out["depth"].detach().float().reshape(1, H, W)
        m = (out["accumulation"].detach().float().reshape(1, H, W) > float(min_alpha)).float()
        return depth_normals((depth * m).contiguous(), m, (camera.fx, camera.fy, camera.cx, camera.cy))

    @torch.no_grad()
    def blur_stats(self, cameras, points: Optional[Tensor] = None):
        """blurscore.BlurStats of `cameras` (one entry per camera, in their order) over `points` [N,3] (default: the
        model's means): how many pixels each frame is smeared and sheared by, as THIS model renders it — every camera's
        effective pose and twist from _viewmat_and_velocity (pose and velocity adjustments included, data velocities
        dropped under zero_initial_velocities) and its effective exposure and readout from shutter_times (the learned
        ones included).  All cameras must share one image size.  On the model's device; no gradient."""
        from .blurscore import blur_stats
        cameras = list(cameras)
        if not cameras:
            raise ValueError("blur_stats needs at least one camera")
        W, H = cameras[0].width, cameras[0].height
        if any((c.width, c.height) != (W, H) for c in cameras):
            raise ValueError("blur_stats needs cameras of one image size")
        dev = self.means.device
        views = [self._viewmat_and_velocity(c) for c in cameras]
        times = [torch.stack(self.shutter_times(c)) for c in cameras]
        intrins = torch.tensor([[c.fx, c.fy, c.cx, c.cy] for c in cameras], dtype=torch.float32).to(dev)
        pts = self.means if points is None else points.to(device=dev, dtype=torch.float32)
        return blur_stats(pts.detach(), *(torch.stack([v[k] for v in views]).detach().float() for k in range(3)), intrins,
                          torch.stack(times).detach().float(), W, H)

    def blur_scores(self, cameras) -> List[float]:
        """one motion_blur_score per camera: blur_stats(cameras).mean_blur, the mean streak length in pixels"""
        return [float(v) for v in self.blur_stats(cameras).mean_blur.tolist()]

    @staticmethod
    def from_scene(config: SplatfactoDeblurConfig, scene: Dict, device, num_cameras: int = 1):
        """Build from a dict with means/log_scales/quats/opacity_logits/sh (e.g. a synthetic scene)."""
        sh = scene["sh"]
        m = SplatfactoDeblurModel(config, scene["means"], scene["log_scales"], scene["quats"],
                                  scene["opacity_logits"], sh[:, 0, :], sh[:, 1:, :], num_cameras)
        return m.to(device)

    @staticmethod
    def from_seed_points(config: SplatfactoDeblurConfig, xyz: Tensor, rgb: Tensor, device, num_cameras: int = 1,
                         seed: int = 0, min_scale: float = 1e-4):
        """splatfacto's initialisation from a seed cloud (xyz [N,3], rgb [N,3] in 0..1; e.g. data.load_seed_points_ply):
        isotropic scale = the mean distance to the 3 nearest neighbours, clamped to min_scale; random unit quaternions from
        torch.Generator().manual_seed(seed); opacity 0.1; colour -> SH dc.  The neighbour search (knn.py) runs on
        `device` and is linear in memory, so the cloud of a real capture (10^5..10^6 points) fits."""
        import math
        from .knn import knn_mean_distance
        xyz = xyz.detach().to(torch.float32).cpu().contiguous()
        n = int(xyz.shape[0])
        g = torch.Generator().manual_seed(seed)
        mean_d = knn_mean_distance(xyz.to(device), 3).cpu()
        log_scales = torch.log(mean_d.clamp(min=min_scale))[:, None].repeat(1, 3)
        quats = torch.randn(n, 4, generator=g)
        quats = quats / quats.norm(dim=-1, keepdim=True)
        sh = torch.zeros(n, (config.sh_degree + 1) ** 2, 3)
        sh[:, 0, :] = (rgb.detach().cpu() - 0.5) / SH_C0
        scene = dict(means=xyz.clone(), log_scales=log_scales, quats=quats,
                     opacity_logits=torch.full((n,), math.log(0.1 / 0.9)), sh=sh)
        return SplatfactoDeblurModel.from_scene(config, scene, device, num_cameras=num_cameras)

    @staticmethod
    def from_random(config: SplatfactoDeblurConfig, device, num_points: int = 50000, scale: float = 10.0,
                    num_cameras: int = 1, seed: int = 0):
        """splatfacto's random start (random_init / num_random / random_scale) for a scene without a seed cloud: means
        uniform in the cube of side `scale` about the origin, uniform colours, the rest as from_seed_points; every draw
        comes from torch.Generator().manual_seed(seed)"""
        g = torch.Generator().manual_seed(seed)
        xyz = (torch.rand(num_points, 3, generator=g) - 0.5) * scale
        rgb = torch.rand(num_points, 3, generator=g)
        return SplatfactoDeblurModel.from_seed_points(config, xyz, rgb, device, num_cameras=num_cameras, seed=seed)

    @staticmethod
    def from_ply(path, config: Optional[SplatfactoDeblurConfig] = None, device="cpu", num_cameras: int = 1):
        """Build from a Gaussian-splat PLY (checkpoint.export_ply / the 3DGS viewers' format): config None = the
        defaults at the file's SH degree.  Camera-side parameters and bilateral grids are not in a PLY."""
        from .checkpoint import model_from_ply
        return model_from_ply(path, config, device, num_cameras)
