"""Forward + backward of one frame as ONE host call, without the autograd engine (round 4).

`ops.render_combined` is an autograd node: a training iteration then crosses Python's autograd machinery between the
forward and the backward compositor — the engine's worker-thread hand-off, the loss's own nodes, allocator calls —
while the GPU queue is EMPTY (the forward ends with a host read-back).  On the 1M-Gaussian benchmark frame that window
was ~0.1 ms of a 2.2 ms step.  `render_step` issues the same C-ABI calls (the plain functions the autograd nodes wrap,
ops.frame_forward / frame_backward and ops.subpose_forward / subpose_backward, called directly) back to back: sub-pose
viewmats -> projection -> frame forward -> sub-frame average -> [d loss / d image] -> frame backward -> projection
backward -> sub-pose backward.  Results are bit-identical to the autograd route (tests/test_gpu_parity.py::
test_render_step_equals_autograd_route); what the loss contributes is either a fixed gradient image or a callable
(e.g. the HIP L1 + SSIM kernel of fused.py, whose forward already produces the gradient).
"""
from __future__ import annotations

from typing import Callable, Dict, Optional, Tuple, Union

import torch
from torch import Tensor

from . import ops


@torch.no_grad()
def render_step(means: Tensor, scales: Tensor, quats: Tensor, opacities: Tensor, sh: Tensor, viewmat: Tensor,
                lin_vel: Tensor, ang_vel: Tensor, times: Tensor, background: Optional[Tensor], blur_samples: int,
                rs_bands: int, fx: float, fy: float, cx: float, cy: float, img_height: int, img_width: int,
                grad_image: Union[Tensor, Callable[[Tensor], Tensor]], gamma: float = 1.0, min_rgb_level: float = 0.0,
                sh_degree: int = 3, antialiased: bool = True, sh_rest: Optional[Tensor] = None, raw_params: bool = True,
                motion_model: str = "se3", xy_grad_out: Optional[Tensor] = None, camera_grads: bool = True,
                background_grad: bool = False, glob_scale: float = 1.0, clip_thresh: float = 0.01,
                rolling_shutter_time: float = 0.0, shared_list: bool = False, hints: Optional["ops.FrameHints"] = None,
                grad_depth: Optional[Union[Tensor, Callable[[Tensor, Tensor], Tuple[Tensor, Optional[Tensor]]]]] = None,
                xy_absgrad_out: Optional[Tensor] = None, times_grad: bool = False
                ) -> Tuple[Tensor, Dict[str, Optional[Tensor]], Tensor]:
    """One frame, forward and backward.  Arguments as ops.render_combined (raw_params: log-scales / opacity logits;
    sh_rest: features_rest beside sh = features_dc), but the camera comes as ONE mid-exposure `viewmat` [4,4] + body
    twist + the P sub-pose `times` for both motion models.  grad_image: d loss / d rgb [H,W,3], or a callable
    rgb -> d loss / d rgb that is invoked between the two halves.
    -> (rgb [H,W,3], gradients {means, scales, quats, opacities, sh, sh_rest, viewmat, lin_vel, ang_vel, background},
        radii [P,N] ([1,N] with shared_list, see ops.render_subposes)) — gradients of exactly the tensors handed in (raw parameters with raw_params=True).
    grad_depth (optional; None: the step is unchanged, launch for launch): a depth loss on the per-sample depth sums
    depth_acc [S,H,W] (sum over the blended splats of weight * camera-space depth, ops.render_subposes return_depth).
    Either d loss / d depth_acc [S,H,W] as a tensor, or a callable (depth_acc [S,H,W], alphas [S,H,W]) ->
    (d loss / d depth_acc, d loss / d alphas or None), invoked between the two halves like grad_image — a loss on the
    expected depth depth_acc / alpha needs the alpha term (SplatfactoDeblurModel.render_and_backward does that chain).
    xy_absgrad_out (optional float32 [N,2], motion_model "se3" only): OVERWRITTEN with the absgrad statistic, as in
    ops.render_subposes; the pixel-velocity model raises ValueError before any launch.
    times_grad=True (motion_model "se3" only): the gradient dict gains "times" [P], d loss / d times, from the same
    sub-pose backward call (gs_subpose_viewmats_bwd_times; the other camera gradients keep their bits).  The
    pixel-velocity model, the shared list and exact rolling shutter raise ValueError before any launch — the times enter
    their projection and compositors, not subpose_viewmats.  False: exactly the keys listed above."""
    S, R = max(1, int(blur_samples)), max(1, int(rs_bands))
    pixvel = motion_model == "pixel_velocity"
    if not pixvel and motion_model != "se3":
        raise ValueError(f"unknown motion_model {motion_model!r}")
    if times_grad and (pixvel or shared_list or float(rolling_shutter_time) != 0.0):
        raise ValueError("times_grad is available with the SE(3) motion model only: the pixel-velocity model, the shared "
                         "list and exact rolling shutter take the sub-pose times inside their projection / compositors")
    depth = grad_depth is not None                      # the alphas are returned for the depth loss only
    spec = ops.FrameSpec.of(S, R, fx, fy, cx, cy, img_height, img_width, sh_degree=sh_degree, antialiased=antialiased,
                            glob_scale=glob_scale, clip_thresh=clip_thresh, gamma=gamma, min_rgb_level=min_rgb_level,
                            return_alpha=depth, return_depth=depth, rs_time=rolling_shutter_time, raw_params=raw_params,
                            shared_list=shared_list)
    ops._validate_frame(pixvel=pixvel, R=R, rs_time=spec.rs_time, shared_list=spec.shared_list,
                        absgrad=xy_absgrad_out is not None, batch=False)
    sub_saved = None
    if pixvel:
        vms = viewmat
    else:
        vms, sub_saved = ops.subpose_forward(viewmat, lin_vel, ang_vel, times)
    want = {"gaussians": True, "viewmats": camera_grads or times_grad, "twist": camera_grads and pixvel,
            "background": background is not None and background_grad, "sh_rest": sh_rest is not None}
    (rgb, alphas, radii, depth_acc), state, saved = ops.frame_forward(
        spec, means, scales, quats, opacities, sh, sh_rest=sh_rest, viewmats=vms, background=background,
        lin_vel=lin_vel if pixvel else None, ang_vel=ang_vel if pixvel else None,
        want=frozenset(k for k, v in want.items() if v), times=times if pixvel else None, xy_grad_out=xy_grad_out,
        xy_absgrad_out=xy_absgrad_out, hints=hints)
    if callable(grad_image):
        # the callable may use torch.autograd itself (rgb.requires_grad_() + autograd.grad): it sees a detached leaf and
        # runs with gradient recording on (under this function's no_grad it silently got None)
        with torch.enable_grad():
            v_rgb = grad_image(rgb.detach())
        if v_rgb is None:
            raise ValueError("grad_image(rgb) returned None: it must return d loss / d rgb [H,W,3]")
        v_rgb = v_rgb.detach()
    else:
        v_rgb = grad_image
    v_alpha = v_depth = None
    if callable(grad_depth):
        with torch.enable_grad():
            res = grad_depth(depth_acc.detach(), alphas.detach())
        if not isinstance(res, (tuple, list)) or len(res) != 2 or res[0] is None:
            raise ValueError("grad_depth(depth_acc, alphas) must return (d loss / d depth_acc [S,H,W], "
                             "d loss / d alphas [S,H,W] or None)")
        v_depth = res[0].detach()
        v_alpha = None if res[1] is None else res[1].detach()
    elif grad_depth is not None:
        v_depth = grad_depth
    if v_depth is not None and tuple(v_depth.shape) != (S, img_height, img_width):
        raise ValueError(f"d loss / d depth_acc must be [S,H,W] = {(S, img_height, img_width)}, got {tuple(v_depth.shape)}")
    g = ops.frame_backward(state, saved, v_rgb, v_alpha, v_depth)
    grads = {"means": g.means, "scales": g.scales, "quats": g.quats, "opacities": g.opacities, "sh": g.sh,
             "background": g.background, "sh_rest": g.sh_rest, "viewmat": None, "lin_vel": None, "ang_vel": None}
    if times_grad:
        grads["times"] = None
    if pixvel:
        grads["viewmat"], grads["lin_vel"], grads["ang_vel"] = g.viewmats, g.lin_vel, g.ang_vel
    elif (camera_grads or times_grad) and g.viewmats is not None:
        v_V, v_lin, v_ang, v_times = ops.subpose_backward(sub_saved, g.viewmats, bool(times_grad))
        if camera_grads:
            grads["viewmat"], grads["lin_vel"], grads["ang_vel"] = v_V, v_lin, v_ang
        if times_grad:
            grads["times"] = v_times
    return rgb, grads, radii
