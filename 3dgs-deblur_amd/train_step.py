"""Loss + optimizer step around the hot path: what the nerfstudio fork's trainer
does right after `get_outputs` — splatfacto's `0.8*L1 + 0.2*(1-SSIM)` image loss, the scale
regularisation switched on by /root/reference/train.py:120 (`use-scale-regularization`), and one Adam
step per parameter group.  On the GPU the loss (forward + backward) and the optimizer step are HIP kernels
(:mod:`fused`, csrc/train.hip): two tile kernels instead of nine conv2d launches plus their autograd graph, one
multi-tensor Adam launch instead of six foreach passes.  The torch formulations below are the same math for CPU
tensors (the gloo host-logic tests drive `train_step` with a CPU stand-in for the render) and the oracle the HIP
kernels are tested against; a CUDA tensor never takes them silently — `image_loss` / `make_optimizers` choose by
device and the HIP side raises when the library is missing.
"""
from __future__ import annotations

import dataclasses
import functools
import math
import os
from typing import Callable, Dict, List, Optional

import torch
import torch.nn.functional as F
from torch import Tensor

from .model import Camera, SplatfactoDeblurModel


def _gauss_window(size: int = 11, sigma: float = 1.5, device=None, dtype=torch.float32) -> Tensor:
    x = torch.arange(size, dtype=torch.float32, device=device) - (size - 1) / 2.0
    g = torch.exp(-(x * x) / (2 * sigma * sigma))
    g = (g / g.sum()).to(dtype)          # the window is built in float32 (as pytorch_msssim does), whatever the images
    return (g[:, None] * g[None, :])[None, None]


def ssim(img: Tensor, ref: Tensor, window: int = 11) -> Tensor:
    """Mean SSIM of two [H,W,3] images in [0,1] (Gaussian 11x11 window, sigma 1.5, valid padding)."""
    x = img.permute(2, 0, 1)[None]
    y = ref.permute(2, 0, 1)[None]
    w = _gauss_window(window, 1.5, img.device, img.dtype).expand(3, 1, window, window)
    mu_x, mu_y = F.conv2d(x, w, groups=3), F.conv2d(y, w, groups=3)
    sxx = F.conv2d(x * x, w, groups=3) - mu_x * mu_x
    syy = F.conv2d(y * y, w, groups=3) - mu_y * mu_y
    sxy = F.conv2d(x * y, w, groups=3) - mu_x * mu_y
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    s = ((2 * mu_x * mu_y + c1) * (2 * sxy + c2)) / ((mu_x * mu_x + mu_y * mu_y + c1) * (sxx + syy + c2))
    return s.mean()


def psnr(img: Tensor, ref: Tensor) -> float:
    mse = torch.mean((img.clamp(0, 1) - ref.clamp(0, 1)) ** 2).item()
    return float("inf") if mse == 0 else -10.0 * math.log10(mse)


# A/B switch: GSD_TORCH_TRAIN=1 runs the loss as torch ops and the optimizers as torch.optim.Adam on the GPU too
TORCH_TRAIN = int(os.environ.get("GSD_TORCH_TRAIN", "0"))


def image_loss(pred: Tensor, gt: Tensor, ssim_lambda: float = 0.2) -> Tensor:
    if pred.is_cuda and not TORCH_TRAIN:
        from . import fused
        return fused.image_loss(pred, gt, ssim_lambda)
    return image_loss_torch(pred, gt, ssim_lambda)


def image_loss_torch(pred: Tensor, gt: Tensor, ssim_lambda: float = 0.2) -> Tensor:
    """the same loss in plain torch ops (CPU tensors; reference for the HIP kernels' tests)"""
    l1 = torch.abs(gt - pred).mean()
    if ssim_lambda <= 0:
        return l1
    return (1.0 - ssim_lambda) * l1 + ssim_lambda * (1.0 - ssim(pred, gt))


def downscale_image(img: Tensor, d: int) -> Tensor:
    """[H,W,3] -> [H//d, W//d, 3] by averaging d x d blocks: splatfacto's `_downscale_if_required` / `resize_image`
    (a stride-d convolution with uniform weights) applied to the ground truth while the resolution schedule is active"""
    if d <= 1:
        return img
    return F.avg_pool2d(img.permute(2, 0, 1)[None], kernel_size=d, stride=d)[0].permute(1, 2, 0).contiguous()


def downscale_depth(depth: Tensor, d: int) -> Tensor:
    """[H,W,1] depth map (0 = no measurement) -> [H//d, W//d, 1]: per d x d block the mean of its VALID samples, 0 where
    the block holds none (the depth counterpart of downscale_image: an invalid pixel never drags a block towards 0)"""
    if d <= 1:
        return depth
    x = depth.permute(2, 0, 1)[None]
    valid = (x > 0).to(x.dtype)
    s = F.avg_pool2d(x * valid, kernel_size=d, stride=d)
    n = F.avg_pool2d(valid, kernel_size=d, stride=d)
    return torch.where(n > 0, s / torch.clamp(n, min=1e-12), torch.zeros_like(s))[0].permute(1, 2, 0).contiguous()


def depth_loss(depth: Tensor, gt_depth: Tensor, depth_lambda: float) -> Tensor:
    """depth_lambda * mean over the pixels with gt_depth > 0 of |depth - gt_depth| (0 without a valid pixel); depth,
    gt_depth [H,W,1] in scene units"""
    valid = (gt_depth > 0).to(depth.dtype)
    n = torch.clamp(valid.sum(), min=1.0)
    return depth_lambda * (torch.abs(depth - gt_depth) * valid).sum() / n


DEPTH_LOSSES = (None, "l1", "pearson")
DEPTH_SPACES = ("depth", "disparity")


def _check_depth_prior(depth_loss, depth_space) -> None:
    """train_step's depth_loss= / depth_space= names, checked before anything is launched"""
    if depth_loss not in DEPTH_LOSSES:
        raise ValueError(f"unknown depth_loss {depth_loss!r} (one of {DEPTH_LOSSES})")
    if depth_space not in DEPTH_SPACES:
        raise ValueError(f"unknown depth_space {depth_space!r} (one of {DEPTH_SPACES})")


def depth_prior_term(depth: Tensor, accumulation: Tensor, prior: Tensor, kind: str, space: str, weight: float) -> Tensor:
    """depthprior.depth_prior_loss of a rendered depth map (autograd and batch routes): depth, accumulation, prior
    [H,W,1]; depth_acc = depth * m, alphas = m with m = (accumulation > 0), one sample, so that x is the depth itself"""
    from .depthprior import depth_prior_loss
    H, W = int(depth.shape[0]), int(depth.shape[1])
    m = (accumulation > 0).to(depth.dtype).reshape(1, H, W)
    return depth_prior_loss(depth.reshape(1, H, W) * m, m, prior.reshape(H, W), kind, space, weight)


def downscale_normals(normals: Tensor, d: int) -> Tensor:
    """[H,W,3] normal map (a zero or non-finite vector = no value) -> [H//d, W//d, 3]: per d x d block the mean of its VALID
    vectors, renormalised; zero where the block holds none or they cancel (the normal counterpart of downscale_depth)"""
    if d <= 1:
        return normals
    valid = torch.isfinite(normals).all(dim=-1, keepdim=True) & (normals != 0).any(dim=-1, keepdim=True)
    x = torch.where(valid, normals, torch.zeros_like(normals)).permute(2, 0, 1)[None]
    s = F.avg_pool2d(x, kernel_size=d, stride=d)[0].permute(1, 2, 0)
    length = s.norm(dim=-1, keepdim=True)
    return torch.where(length > 0, s / torch.clamp(length, min=1e-30), torch.zeros_like(s)).contiguous()


def _check_normal_term(gt_normal, normal_lambda, normal_smooth_lambda, normal_edge_beta) -> None:
    """train_step's normal keywords, checked before anything is launched"""
    for name, v in (("normal_lambda", normal_lambda), ("normal_smooth_lambda", normal_smooth_lambda),
                    ("normal_edge_beta", normal_edge_beta)):
        if not (float(v) >= 0.0 and math.isfinite(float(v))):
            raise ValueError(f"{name} must be a finite number >= 0, got {v}")
    for g in (gt_normal if isinstance(gt_normal, (list, tuple)) else [gt_normal]):
        if g is not None and not (isinstance(g, Tensor) and g.dim() == 3 and g.shape[-1] == 3):
            raise ValueError(f"gt_normal must be a [H,W,3] tensor, got {tuple(g.shape) if isinstance(g, Tensor) else type(g)}")


def _camera_intrins(model: SplatfactoDeblurModel, camera: Camera):
    """fx, fy, cx, cy of the camera the frame is rendered with: the rescaled one under the resolution schedule"""
    d = model.downscale_factor()
    cam = camera.rescaled(d) if d > 1 else camera
    return (cam.fx, cam.fy, cam.cx, cam.cy)


def normal_term(depth: Tensor, accumulation: Tensor, intrins, prior: Optional[Tensor], guide: Optional[Tensor],
                prior_weight: float, smooth_weight: float, edge_beta: float) -> Tensor:
    """normals.normal_loss of a rendered depth map (autograd and batch routes): depth, accumulation [H,W,1], prior / guide
    [H,W,3] or None; depth_acc = depth * m, alphas = m with m = (accumulation > 0), one sample, as depth_prior_term"""
    from .normals import normal_loss
    H, W = int(depth.shape[0]), int(depth.shape[1])
    m = (accumulation > 0).to(depth.dtype).reshape(1, H, W)
    return normal_loss(depth.reshape(1, H, W) * m, m, intrins, prior, guide, prior_weight if prior is not None else 0.0,
                       smooth_weight, edge_beta)


def _metric_depth_sums(depth_acc: Tensor, alphas: Tensor, gt_depth: Tensor, depth_lambda: float):
    """the metric depth L1 as a loss on the compositor's raw sums: (loss, d loss / d depth_acc, d loss / d alphas) — what
    render_and_backward builds for grad_depth, for a sums callable that also carries another term"""
    from .model import expected_depth
    da, al = depth_acc.detach().requires_grad_(True), alphas.detach().requires_grad_(True)
    dl = depth_loss(expected_depth(da, al), gt_depth, depth_lambda)
    v_acc, v_al = torch.autograd.grad(dl, (da, al), allow_unused=True)
    return (dl.detach(), torch.zeros_like(da) if v_acc is None else v_acc, torch.zeros_like(al) if v_al is None else v_al)


@dataclasses.dataclass
class GeometryTerm:
    """One loss on a camera's rendered geometry, in the two forms train_step's routes need"""
    name: str                      # the key its value is logged under
    on_sums: Callable              # (depth_acc, alphas [S,H,W]) -> (loss, v_depth_acc, v_alphas): the one-call route
    on_map: Callable               # (depth, accumulation [H,W,1]) -> loss, differentiable: the autograd and batch routes
    native_sums: bool = True       # False: on_sums is only an autograd chain around on_map (the metric L1)


def geometry_terms(model: SplatfactoDeblurModel, camera: Camera, gt_image: Tensor, gt_depth: Optional[Tensor],
                   depth_lambda: float, depth_kind: Optional[str], depth_space: str, gt_normal: Optional[Tensor],
                   normal_lambda: float, normal_smooth_lambda: float, normal_edge_beta: float) -> List[GeometryTerm]:
    """train_step's geometry keywords for ONE camera -> its terms, in the order every route adds them: the depth term
    (gt_depth with depth_lambda > 0: the metric L1 for depth_kind None, else depthprior's loss of that kind), then the normal
    term (gt_normal with normal_lambda > 0 and / or normal_smooth_lambda > 0; without a prior its weight reaches the op as
    0.0).  A missing map gives no such term.  gt_image: the target at the render's resolution; it is the edge guide when
    normal_edge_beta > 0.  The maps are moved to its device and follow the resolution schedule, the intrinsics are those
    of the rescaled camera."""
    d = model.downscale_factor()
    terms = []
    if gt_depth is not None and depth_lambda > 0:
        gt = downscale_depth(gt_depth.to(gt_image.device, torch.float32), d)
        if depth_kind is None:
            terms.append(GeometryTerm("depth_loss", lambda acc, al: _metric_depth_sums(acc, al, gt, depth_lambda),
                                      lambda depth, _accumulation: depth_loss(depth, gt, depth_lambda), native_sums=False))
        else:
            from .depthprior import depth_prior_loss_with_grad
            prior, d_args = gt.reshape(gt.shape[0], gt.shape[1]), (depth_kind, depth_space, depth_lambda)
            terms.append(GeometryTerm("depth_loss", lambda acc, al: depth_prior_loss_with_grad(acc, al, prior, *d_args),
                                      lambda depth, accumulation: depth_prior_term(depth, accumulation, gt, *d_args)))
    use_prior = gt_normal is not None and normal_lambda > 0
    if use_prior or normal_smooth_lambda > 0:
        from .normals import normal_loss_with_grad
        normals = downscale_normals(gt_normal.to(gt_image.device, torch.float32), d) if use_prior else None
        n_args = (_camera_intrins(model, camera), normals, gt_image if normal_edge_beta > 0 else None,
                  normal_lambda if use_prior else 0.0, normal_smooth_lambda, normal_edge_beta)
        terms.append(GeometryTerm("normal_loss", lambda acc, al: normal_loss_with_grad(acc, al, *n_args),
                                  lambda depth, accumulation: normal_term(depth, accumulation, *n_args)))
    return terms


def scale_regularization(log_scales: Tensor, max_gauss_ratio: float = 10.0) -> Tensor:
    """Penalise needle-like Gaussians (PhysGaussian-style, as in splatfacto): mean(max(s_max/s_min, r) - r)."""
    s = torch.exp(log_scales)
    ratio = s.amax(dim=-1) / s.amin(dim=-1)
    r = torch.tensor(max_gauss_ratio, device=s.device, dtype=s.dtype)
    return 0.1 * (torch.maximum(ratio, r) - r).mean()


def mcmc_regularization(opacity_logits: Tensor, log_scales: Tensor, opacity_reg: float, scale_reg: float) -> Tensor:
    """3DGS-MCMC's two regularisers (gsplat's MCMC trainer, recollected; upstream uses 0.01 for both):
    opacity_reg * mean(sigmoid(opacities)) + scale_reg * mean(exp(scales)).  They are what lets Gaussians die."""
    reg = opacity_logits.new_zeros(())
    if opacity_reg:
        reg = reg + opacity_reg * torch.sigmoid(opacity_logits).mean()
    if scale_reg:
        reg = reg + scale_reg * torch.exp(log_scales).mean()
    return reg


def _small_params(model: SplatfactoDeblurModel):
    """the parameters that are not per-Gaussian rows — learnable background, pose / velocity adjustments, bilateral
    grids, exposure / readout adjustments: under data parallelism their gradients travel in one small dense bucket"""
    return [p for p in (model.background_param, model.pose_adjustment, model.velocity_adjustment,
                        getattr(model, "bilateral_grids", None), getattr(model, "exposure_adjustment", None),
                        getattr(model, "readout_adjustment", None)) if p is not None]


def _grid_tv(model: SplatfactoDeblurModel) -> Optional[Tensor]:
    """bilateral_grid_tv_lambda * tv(all grids) as a differentiable loss term, or None without grids / with lambda 0"""
    grids = getattr(model, "bilateral_grids", None)
    lam = float(model.config.bilateral_grid_tv_lambda) if grids is not None else 0.0
    if grids is None or lam == 0.0:
        return None
    from . import bilagrid
    return bilagrid.tv_loss(grids, lam)


def _mcmc_reg(model: SplatfactoDeblurModel) -> Optional[Tensor]:
    """the MCMC regularisers of model.config, or None when both are 0.0 (nothing is built)"""
    cfg = model.config
    if not (cfg.opacity_reg or cfg.scale_reg):
        return None
    return mcmc_regularization(model.opacities, model.scales, cfg.opacity_reg, cfg.scale_reg)


def _add_regularizers(model: SplatfactoDeblurModel, loss: Tensor) -> Tensor:
    """loss + the scale, MCMC and grid-TV regularisers model.config switches on, as differentiable terms (the autograd and
    batch routes; the one-call route runs its own backward per term)"""
    if model.config.use_scale_regularization:
        loss = loss + scale_regularization(model.scales)
    reg = _mcmc_reg(model)
    if reg is not None:
        loss = loss + reg
    tv = _grid_tv(model)
    if tv is not None:
        loss = loss + tv
    return loss


class SelectiveAdam(torch.optim.Optimizer):
    """Selective ("visibility-masked") Adam in plain torch: gsplat's SelectiveAdam / Taming-3DGS's sparse optimizer.
    step(row_mask) runs torch.optim.Adam's update (no weight decay, no amsgrad; state keys and the tensor step count
    as torch's) on the rows r with row_mask[r] only, for every parameter whose leading dimension is row_mask's length;
    the other rows keep parameter, exp_avg and exp_avg_sq unchanged and their gradient is ignored.  The step count
    advances every step and bias correction uses it (gsplat's rule: no per-row step count).  row_mask=None is a dense
    torch.optim.Adam step.  The CPU / A/B form of fused.adam_step_all(row_mask=...) and its test oracle."""
    selective = True

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))

    @torch.no_grad()
    def step(self, row_mask: Optional[Tensor] = None, closure=None):
        for group in self.param_groups:
            beta1, beta2 = group["betas"]
            lr, eps = group["lr"], group["eps"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
                step = float(st["step"])
                bias_correction1 = 1 - beta1 ** step
                bias_correction2 = 1 - beta2 ** step
                step_size = lr / bias_correction1
                bias_correction2_sqrt = bias_correction2 ** 0.5
                exp_avg, exp_avg_sq = st["exp_avg"], st["exp_avg_sq"]
                idx = None
                if row_mask is not None and p.dim() >= 1 and p.shape[0] == row_mask.numel():
                    idx = row_mask.to(device=p.device, dtype=torch.bool).nonzero().reshape(-1)
                if idx is None:
                    q, g, m, v = p, p.grad, exp_avg, exp_avg_sq
                else:
                    q, g, m, v = (t.index_select(0, idx) for t in (p, p.grad, exp_avg, exp_avg_sq))
                m.lerp_(g, 1 - beta1)
                v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
                denom = (v.sqrt() / bias_correction2_sqrt).add_(eps)
                q.addcdiv_(m, denom, value=-step_size)
                if idx is not None:
                    p.index_copy_(0, idx, q)
                    exp_avg.index_copy_(0, idx, m)
                    exp_avg_sq.index_copy_(0, idx, v)


OPTIMIZERS = ("adam", "selective_adam")
# learning rate of the "camera_shutter_opt" group (log-seconds per step): measured, DESIGN §5.9
SHUTTER_LR = 1e-3


def shutter_params(model: SplatfactoDeblurModel):
    """the exposure / readout adjustments the model holds (SplatfactoDeblurConfig.camera_shutter_optimizer), in that order"""
    return [p for p in (getattr(model, "exposure_adjustment", None), getattr(model, "readout_adjustment", None))
            if p is not None]
SELECTIVE_MASKS = ("visible", "touched")


def make_optimizers(model: SplatfactoDeblurModel, lr_scale: float = 1.0,
                    fused: Optional[bool] = None, optimizer: Optional[str] = None) -> Dict[str, torch.optim.Optimizer]:
    """One Adam per parameter group with splatfacto's default learning rates.  fused (default: the parameters live on
    a GPU): HipAdam — same update rule and state layout as torch.optim.Adam, stepped by ONE multi-tensor HIP launch
    (`optimizers_step`); False: torch.optim.Adam (CPU tensors, A/B).
    optimizer (default: model.config.optimizer): "adam", or "selective_adam" — the six Gaussian groups then step only
    the rows of train_step's row mask (model.config.selective_mask): HipAdam(selective=True) through
    gs_adam_step_rows, or SelectiveAdam when not fused.  Pose, velocity and background optimizers stay dense."""
    lrs = {"means": 1.6e-4, "scales": 5e-3, "quats": 1e-3, "opacities": 5e-2, "features_dc": 2.5e-3,
           "features_rest": 2.5e-3 / 20}
    optimizer = model.config.optimizer if optimizer is None else optimizer
    if optimizer not in OPTIMIZERS:
        raise ValueError(f"unknown optimizer {optimizer!r} (one of {OPTIMIZERS})")
    selective = optimizer == "selective_adam"
    if fused is None:
        fused = model.means.is_cuda and not TORCH_TRAIN
    if fused:
        from .fused import HipAdam as Adam
        GaussAdam = functools.partial(Adam, selective=True) if selective else Adam
    else:
        Adam = torch.optim.Adam
        GaussAdam = SelectiveAdam if selective else Adam
    opts = {k: GaussAdam([p], lr=lrs[k] * lr_scale, eps=1e-15) for k, p in model.gauss_params().items()}
    if model.pose_adjustment is not None:
        opts["camera_opt"] = Adam([model.pose_adjustment], lr=1e-4 * lr_scale, eps=1e-15)
    if model.velocity_adjustment is not None:
        opts["camera_velocity_opt"] = Adam([model.velocity_adjustment], lr=1e-3 * lr_scale, eps=1e-15)
    if model.background_param is not None:
        opts["background"] = Adam([model.background_param], lr=1e-3 * lr_scale, eps=1e-15)
    if model.bilateral_grids is not None:
        # splatfacto's bilateral_grid group (2e-3, eps 1e-15); upstream warms it up and decays it — this trainer has no
        # schedulers
        opts["bilateral_grid"] = Adam([model.bilateral_grids], lr=2e-3 * lr_scale, eps=1e-15)
    shutter = shutter_params(model)
    if shutter:
        # learnable exposure / readout times (log-scale adjustments): one dense group for whichever exist
        opts["camera_shutter_opt"] = Adam(shutter, lr=SHUTTER_LR * lr_scale, eps=1e-15)
    return opts


def optimizers_step(optimizers, row_mask: Optional[Tensor] = None) -> None:
    """step every optimizer of the iteration; HipAdam instances share one multi-tensor launch.  row_mask (bool [N]):
    selective Adam — the per-Gaussian groups step only the selected rows (fused.adam_step_all / SelectiveAdam)"""
    opts = list(optimizers)
    if any(type(o).__name__ == "HipAdam" for o in opts):
        from .fused import adam_step_all
        if row_mask is None:
            adam_step_all(opts)
        else:
            adam_step_all(opts, row_mask=row_mask)
    else:
        for o in opts:
            if row_mask is not None and getattr(o, "selective", False):
                o.step(row_mask)
            else:
                o.step()


def selection_mask(model: SplatfactoDeblurModel, optimizers, allreduce: Optional[str] = None) -> Optional[Tensor]:
    """The row mask of a selective-Adam step (bool [N]), or None when no optimizer of the step is selective (plain
    Adam: nothing is built).  Call after the backward and after any DP gradient exchange.
    model.config.selective_mask "visible": rows with radii > 0 in any sub-pose of any camera of the step (model.radii;
    gs_visible_rows), made identical on every rank by a MAX all-reduce under data parallelism; "touched": rows with
    any non-zero gradient in any Gaussian parameter (gs_dp_row_mask), read from the exchanged gradients, hence
    identical on every rank with no collective of its own."""
    if not any(getattr(o, "selective", False) for o in optimizers):
        return None
    kind = model.config.selective_mask
    N = model.num_points
    dev = model.means.device
    if kind == "touched":
        grads = [p.grad.contiguous() for p in model.gauss_params().values() if p.grad is not None]
        if N == 0 or not grads:
            return torch.zeros(N, dtype=torch.bool, device=dev)
        from .dp import _RowOps
        return _RowOps(grads).row_mask()
    if kind != "visible":
        raise ValueError(f"unknown selective_mask {kind!r} (one of {SELECTIVE_MASKS})")
    radii = model.radii
    if radii is None:
        raise RuntimeError("selective_mask='visible' needs the step's radii (model.radii): render before the step")
    planes = [r.reshape(-1, r.shape[-1]) for r in (radii if isinstance(radii, (list, tuple)) else [radii])]
    if any(r.shape[-1] != N for r in planes):
        raise RuntimeError(f"model.radii has {planes[0].shape[-1]} rows, the model {N}: radii of an earlier step")
    planes = planes[0] if len(planes) == 1 else torch.cat(planes)
    if planes.is_cuda:
        from .fused import visible_rows
        mask = visible_rows(planes.to(torch.int32))
    else:
        mask = (planes > 0).any(dim=0)
    if allreduce is not None:
        from . import dp
        dp.allreduce_mask_max_(mask)
    return mask


# GSD_TRAIN_AUTOGRAD=1: train_step goes through get_outputs + torch.autograd instead of the one-call route (A/B, tests)
TRAIN_AUTOGRAD = int(os.environ.get("GSD_TRAIN_AUTOGRAD", "0"))


def one_call_route(model: SplatfactoDeblurModel) -> bool:
    """train_step renders through model.render_and_backward (step.render_step) unless the model lives on the CPU (host
    logic tests with a stand-in render), the torch loss / autograd A/B switches are set, or training wants get_outputs'
    depth map every step (output_depth_during_training).  A depth LOSS runs on both routes (train_step gt_depth)"""
    return (model.means.is_cuda and not TORCH_TRAIN and not TRAIN_AUTOGRAD
            and not model.config.output_depth_during_training and "get_outputs" not in model.__dict__
            and type(model).get_outputs is SplatfactoDeblurModel.get_outputs)


def train_step(model: SplatfactoDeblurModel, optimizers: Dict[str, torch.optim.Optimizer], camera: Camera,
               gt_image: Tensor, ssim_lambda: float = 0.2, allreduce: Optional[str] = None,
               gt_depth: Optional[Tensor] = None, depth_lambda: float = 0.0, depth_loss: Optional[str] = None,
               depth_space: str = "depth", gt_normal: Optional[Tensor] = None, normal_lambda: float = 0.0,
               normal_smooth_lambda: float = 0.0, normal_edge_beta: float = 0.0) -> Dict[str, float]:
    """One training iteration: render (HIP) -> loss -> backward (HIP) -> [DP gradient all-reduce] -> Adam.
    camera / gt_image (/ gt_depth / gt_normal) may be lists: B cameras rendered as one batch (_train_step_batch), the loss
    the mean over the cameras of the per-image loss, on the autograd route.
    The geometry keywords become one short list of terms per camera (geometry_terms: the depth term, then the normal term);
    every term is added to the image loss and logged in "loss".  The one-call route runs them on the compositor's raw
    per-sample sums between the two halves of the frame (render_and_backward grad_depth_sums: their gradients are added, no
    torch op per term), except that a lone metric L1 travels as grad_depth, the chain on the depth map the step has always
    built for it; the autograd and batch routes run them on the rendered depth map.  What each keyword adds:
    gt_depth [H,W,1] (scene units, 0 = no measurement) with depth_lambda > 0: the depth term — depth_loss None: the metric
    L1 (depth_loss()); "pearson" / "l1": gt_depth is a depth PRIOR and the term depthprior.depth_prior_loss(kind=depth_loss,
    space=depth_space, weight=depth_lambda), "pearson" for a monocular prior known up to scale and shift,
    depth_space="disparity" for one given as inverse depth.
    gt_normal [H,W,3] (a normal PRIOR in the camera frame, x right, y down, z forward; a zero vector = no value) with
    normal_lambda > 0, and / or normal_smooth_lambda > 0 (which needs no prior): the normal term, normals.normal_loss =
    normal_lambda * mean(1 - n.m) + normal_smooth_lambda * mean over adjacent pairs of g (1 - n_p.n_q) on the normals of
    the rendered depth, with gt_image as the edge guide of g when normal_edge_beta > 0.
    Unknown names and bad weights raise ValueError before anything is launched; with every geometry keyword at its default
    the step is what it was, bit for bit."""
    _check_depth_prior(depth_loss, depth_space)
    _check_normal_term(gt_normal, normal_lambda, normal_smooth_lambda, normal_edge_beta)
    if isinstance(camera, (list, tuple)):
        return _train_step_batch(model, optimizers, list(camera), list(gt_image), ssim_lambda, allreduce,
                                 gt_depth, depth_lambda, depth_loss, depth_space, gt_normal, normal_lambda,
                                 normal_smooth_lambda, normal_edge_beta)
    model.train()
    for o in optimizers.values():
        o.zero_grad(set_to_none=True)
    gt_image = downscale_image(gt_image, model.downscale_factor())     # num_downscales resolution schedule
    terms = geometry_terms(model, camera, gt_image, gt_depth, depth_lambda, depth_loss, depth_space, gt_normal, normal_lambda,
                           normal_smooth_lambda, normal_edge_beta)
    if one_call_route(model):
        # forward + backward of the frame as ONE host call (model.render_and_backward -> step.render_step): the HIP loss
        # kernel's forward already produces d loss / d rgb, so it sits between the two halves as a plain callable
        from . import fused
        box = {}
        grid_index = model._grid_index(camera, None)       # raises on a bad cam_idx before anything is launched

        def grad_image(rgb):
            if grid_index is None:
                box["loss"], v, _ = fused.image_loss_with_grad(rgb, gt_image, ssim_lambda)
                return v
            # slice forward -> loss on the corrected image -> slice backward: d loss / d raw rgb goes back to the
            # compositor, the grid gradient stays on the parameter
            from . import bilagrid
            grids = model.bilateral_grids
            box["rgb"] = corrected = bilagrid.slice_fwd(grids, rgb, grid_index)
            box["loss"], v, _ = fused.image_loss_with_grad(corrected, gt_image, ssim_lambda)
            v_rgb, v_grids = bilagrid.slice_bwd(grids, rgb, grid_index, v)
            grids.grad = v_grids if grids.grad is None else grids.grad + v_grids
            return v_rgb

        def grad_depth(depth, accumulation):               # a lone term without a form of its own on the sums
            depth = depth.requires_grad_(True)
            box[terms[0].name] = dl = terms[0].on_map(depth, accumulation)
            return torch.autograd.grad(dl, depth)[0]

        def grad_depth_sums(depth_acc, alphas):            # the terms in order, their gradient pairs added
            total = None
            for term in terms:
                box[term.name], v_acc, v_al = term.on_sums(depth_acc, alphas)
                total = (v_acc, v_al) if total is None else (total[0] + v_acc, total[1] + v_al)
            return total
        lone_map_term = len(terms) == 1 and not terms[0].native_sums
        depth_kw = {} if not terms else {"grad_depth": grad_depth} if lone_map_term else {"grad_depth_sums": grad_depth_sums}
        rgb = model.render_and_backward(camera, grad_image, **depth_kw)
        rgb = box.get("rgb", rgb)                          # the logged PSNR is of the corrected image
        loss = box["loss"]
        for term in terms:
            loss = loss + box[term.name].detach()
        if model.config.use_scale_regularization:
            reg = scale_regularization(model.scales)
            reg.backward()
            loss = loss + reg.detach()
        reg = _mcmc_reg(model)
        if reg is not None:
            reg.backward()
            loss = loss + reg.detach()
        if model.bilateral_grids is not None and model.config.bilateral_grid_tv_lambda:
            # value and gradient in one kernel call, the gradient added to the parameter's
            from . import bilagrid
            grids = model.bilateral_grids
            if grids.grad is None:
                grids.grad = torch.zeros_like(grids)
            loss = loss + bilagrid.tv_fwd_bwd_hip(grids.detach(), float(model.config.bilateral_grid_tv_lambda), grids.grad)
    else:
        out = model.get_outputs(camera, return_depth=True) if terms else model.get_outputs(camera)
        rgb = out["rgb"].detach()
        loss = image_loss(out["rgb"], gt_image, ssim_lambda)
        for term in terms:
            loss = loss + term.on_map(out["depth"], out["accumulation"])
        loss = _add_regularizers(model, loss)
        loss.backward()
    return _finish_step(model, optimizers, allreduce, loss, lambda: F.mse_loss(rgb.clamp(0, 1), gt_image.clamp(0, 1)))


def _finish_step(model: SplatfactoDeblurModel, optimizers, allreduce: Optional[str], loss: Tensor,
                 mse: Callable[[], Tensor]) -> Dict[str, float]:
    """what follows the backward of a step: [DP gradient all-reduce] -> Adam on the step's rows -> model.step -> the log
    values.  mse: builds the mean squared error of the step's render(s), after the optimizers have been issued"""
    if allreduce is not None:
        _dp_allreduce(model, allreduce)
    optimizers_step(optimizers.values(), row_mask=selection_mask(model, optimizers.values(), allreduce))
    model.step += 1
    # ONE read-back for the step's two log values (each .item() is a stream synchronisation)
    loss_v, mse_v = torch.stack([loss.detach().reshape(()).float(), mse().float()]).tolist()
    return {"loss": float(loss_v), "psnr": float("inf") if mse_v == 0 else -10.0 * math.log10(mse_v)}


def _dp_allreduce(model: SplatfactoDeblurModel, allreduce: str) -> None:
    from . import dp
    dp.allreduce_gradients(list(model.gauss_params().values()), mode=allreduce, average=True)
    # the parameters that are not per-Gaussian rows (learnable background, pose / velocity adjustments) see
    # only this rank's views too: one small dense bucket, or the replicas drift apart silently
    small = _small_params(model)
    for p in small:
        if p.grad is None:
            p.grad = torch.zeros_like(p)
    dp.allreduce_dense_([p.grad for p in small], average=True)


def _train_step_batch(model: SplatfactoDeblurModel, optimizers, cameras, gt_images, ssim_lambda, allreduce,
                      gt_depths, depth_lambda, depth_loss: Optional[str] = None,
                      depth_space: str = "depth", gt_normals=None, normal_lambda: float = 0.0,
                      normal_smooth_lambda: float = 0.0, normal_edge_beta: float = 0.0) -> Dict[str, float]:
    """train_step for B cameras: one get_outputs_batch, loss = mean over the cameras of train_step's per-image loss
    (image loss + the camera's geometry_terms; the keywords as train_step's, gt_depths / gt_normals lists with None for a
    camera without that map), one autograd backward, one optimizer step"""
    _check_depth_prior(depth_loss, depth_space)
    _check_normal_term(gt_normals, normal_lambda, normal_smooth_lambda, normal_edge_beta)
    if len(cameras) != len(gt_images) or not cameras:
        raise ValueError("train_step needs as many images as cameras")
    model.train()
    for o in optimizers.values():
        o.zero_grad(set_to_none=True)
    B = len(cameras)
    gts = [downscale_image(g, model.downscale_factor()) for g in gt_images]
    terms = [geometry_terms(model, cameras[b], gts[b], None if gt_depths is None else gt_depths[b], depth_lambda, depth_loss,
                            depth_space, None if gt_normals is None else gt_normals[b], normal_lambda, normal_smooth_lambda,
                            normal_edge_beta) for b in range(B)]
    out = model.get_outputs_batch(cameras, return_depth=True) if any(terms) else model.get_outputs_batch(cameras)
    losses = []
    for b in range(B):
        l_b = image_loss(out["rgb"][b], gts[b], ssim_lambda)
        for term in terms[b]:
            l_b = l_b + term.on_map(out["depth"][b], out["accumulation"][b])
        losses.append(l_b)
    loss = _add_regularizers(model, torch.stack([l.reshape(()) for l in losses]).mean())
    loss.backward()
    return _finish_step(model, optimizers, allreduce, loss, lambda: torch.stack(
        [F.mse_loss(out["rgb"][b].detach().clamp(0, 1), gts[b].clamp(0, 1)) for b in range(B)]).mean())


# --------------------------------------------------------------------------- #
# whole-scene training / evaluation on a transforms.json dataset (the trainer-side callers of the hot path that the
# end-to-end deblurring check needs; /root/reference/train.py:78-109 scores runs the same way: PSNR / SSIM of the
# evaluation frames plus wall-clock time, stored as metrics.json)
# --------------------------------------------------------------------------- #
def eval_camera_step(model: SplatfactoDeblurModel, optimizers: Dict[str, torch.optim.Optimizer], camera: Camera,
                     gt_image: Tensor, ssim_lambda: float = 0.2) -> float:
    """`--optimize-eval-cameras` (/root/reference/train.py:180-183, README.md:197): one step on an EVALUATION frame
    in which only its pose / velocity adjustment is updated — the Gaussians are constants (no gradient reaches them,
    their optimizers do not step).  The shutter optimizer's exposure / readout adjustments do NOT step either: an
    evaluation frame must not move a global shutter estimate (it renders WITH the learned times; what gradient it
    leaves on the two parameters is cleared before returning, and "per_camera" exposure rows of evaluation cameras
    therefore stay 0)."""
    model.train()
    cam_opts = [optimizers[k] for k in ("camera_opt", "camera_velocity_opt") if k in optimizers]
    if not cam_opts:
        return float("nan")
    for o in cam_opts:
        o.zero_grad(set_to_none=True)
    # an evaluation frame has no bilateral grid of its own to learn: rendered without the colour correction
    no_grid = {"bilateral_grid": False} if getattr(model, "bilateral_grids", None) is not None else {}
    out = model.get_outputs(camera, detach_gaussians=True, **no_grid)
    gt_image = downscale_image(gt_image, model.downscale_factor())
    loss = image_loss(out["rgb"], gt_image, ssim_lambda)
    loss.backward()
    optimizers_step(cam_opts)
    for p in shutter_params(model):
        p.grad = None
    return float(loss.item())


@torch.no_grad()
def evaluate(model: SplatfactoDeblurModel, cameras, images, indices, batch_size: int = 1,
             color_corrected: Optional[bool] = None) -> Dict[str, float]:
    """mean PSNR / SSIM of the model's renders of `indices` against their images (sharp frames in the synthetic sets).
    batch_size > 1 renders up to that many cameras per call (model.get_outputs_for_cameras).  color_corrected (None:
    model.config.color_corrected_metrics): the result gains cc_psnr / cc_ssim, the same two metrics of each render
    (clamped to [0,1]) after colorcorrect.color_correct fitted it to its image — one call per render batch; psnr and ssim
    stay what they are without it"""
    if color_corrected is None:
        color_corrected = bool(model.config.color_corrected_metrics)
    ps, ss, cps, css = [], [], [], []
    indices = list(indices)
    if color_corrected:
        from .colorcorrect import color_correct
    if batch_size > 1:
        rgbs, fitted = [], []
        for k in range(0, len(indices), batch_size):
            ids = indices[k:k + batch_size]
            batch = model.get_outputs_for_cameras([cameras[i] for i in ids])["rgb"]
            rgbs += list(batch)
            if color_corrected:
                fitted += list(color_correct(batch.clamp(0, 1), torch.stack([images[i] for i in ids])))
    for n, i in enumerate(indices):
        rgb = rgbs[n] if batch_size > 1 else model.get_outputs_for_camera(cameras[i])["rgb"]
        ps.append(psnr(rgb, images[i]))
        ss.append(float(ssim(rgb.clamp(0, 1), images[i]).item()))
        if color_corrected:
            cc = fitted[n] if batch_size > 1 else color_correct(rgb.clamp(0, 1), images[i])
            cps.append(psnr(cc, images[i]))
            css.append(float(ssim(cc, images[i]).item()))
    res = {"psnr": sum(ps) / max(1, len(ps)), "ssim": sum(ss) / max(1, len(ss))}
    if color_corrected:
        res.update(cc_psnr=sum(cps) / max(1, len(cps)), cc_ssim=sum(css) / max(1, len(css)))
    return res


def train_scene(model: SplatfactoDeblurModel, scene, images, iterations: int, lr_scale: float = 1.0,
                ssim_lambda: float = 0.2, optimize_eval_cameras: bool = False, eval_camera_every: int = 4,
                densify=None, log_every: int = 0, seed: int = 0, depths=None, depth_lambda: float = 0.0,
                batch_size: int = 1, optimizer: Optional[str] = None, checkpoint_path=None, checkpoint_every: int = 0,
                resume=None, depth_loss: Optional[str] = None, depth_space: str = "depth", normals=None,
                normal_lambda: float = 0.0, normal_smooth_lambda: float = 0.0, normal_edge_beta: float = 0.0) -> Dict:
    """Train on scene.train_indices (one view per step, seeded shuffle), optionally refining the evaluation cameras
    in between; returns {'results': {psnr, ssim}, 'wall_clock_time_seconds', 'history'} like the reference's
    metrics.json (/root/reference/train.py:87-100, parse_outputs.py:58); with config.color_corrected_metrics the results
    also carry cc_psnr / cc_ssim (evaluate).  depths (optional): per-frame depth maps
    [H,W,1] or None, indexed like images (data.load_depth); with depth_lambda > 0 every step adds the depth loss.
    depth_loss / depth_space: train_step's — "pearson" (or "l1") takes the maps as depth PRIORS (depthprior).
    normals (optional): per-frame normal priors [H,W,3] or None, indexed like images (data.load_scene_normals), used with
    normal_lambda > 0; normal_smooth_lambda / normal_edge_beta: train_step's (the smoothness term needs no prior).
    batch_size > 1: every step takes that many views of the shuffle (fewer at the end of a pass) as one batch
    (train_step with lists), and the evaluation renders in batches of that size.  optimizer: make_optimizers' choice
    ("adam" / "selective_adam"; default model.config.optimizer).  densify: a densify.DensifyConfig (splatfacto's split /
    duplicate / cull schedule, driven by the screen-space gradient statistic) or an mcmc.MCMCConfig (fixed-budget
    relocation + per-step noise; no statistic is collected, collect_densify_stats stays off).
    checkpoint_path: checkpoint.save_checkpoint writes model, optimizers, loop state and densification accumulators there
    after the last step, and with checkpoint_every=K also after steps K, 2K, ...  resume=path: restore all of that into
    `model` (same config; its Gaussian parameters are replaced by the saved ones, whatever their row count) and continue
    at the saved iteration + 1 with the saved optimizers (`lr_scale`, `optimizer` and `seed` are then the file's);
    `iterations` stays the total target, and the returned wall_clock_time_seconds and history continue the saved ones.
    Under an initialised process group only rank 0 writes, then all ranks barrier."""
    import time
    from . import mcmc as M
    use_mcmc = isinstance(densify, M.MCMCConfig)
    _check_depth_prior(depth_loss, depth_space)
    _check_normal_term(None, normal_lambda, normal_smooth_lambda, normal_edge_beta)
    normal_kw = dict(normal_lambda=normal_lambda, normal_smooth_lambda=normal_smooth_lambda, normal_edge_beta=normal_edge_beta)
    if checkpoint_every and checkpoint_path is None:
        raise ValueError("checkpoint_every needs checkpoint_path")
    loaded = None
    if resume is not None:
        from . import checkpoint as C
        loaded = C.load_checkpoint(resume, into=model)
        if loaded.optimizers is None or loaded.trainer is None:
            raise ValueError(f"{resume}: a checkpoint without optimizer / trainer state cannot be resumed")
        strategy = None if densify is None else ("mcmc" if use_mcmc else "splatfacto")
        if loaded.trainer.get("strategy") != strategy:
            raise ValueError(f"{resume} was trained with densify strategy {loaded.trainer.get('strategy')!r}, "
                             f"this call asks for {strategy!r}")
        optimizers = loaded.optimizers
    else:
        optimizers = make_optimizers(model, lr_scale, optimizer=optimizer)
    g = torch.Generator().manual_seed(seed)
    order = []
    history = []
    t0 = time.time()
    state = None
    if densify is not None and not use_mcmc:
        from . import densify as D
        model.collect_densify_stats = True
        if densify.absgrad and not model.config.densify_absgrad:
            raise ValueError("DensifyConfig.absgrad needs a model with SplatfactoDeblurConfig.densify_absgrad=True")
        state = D.DensifyState(model.num_points, model.means.device, densify.absgrad)
        if densify.num_train_data <= 0:
            # upstream's post-reset guard counts in passes over the training images (nerfstudio sets num_train_data
            # from the datamanager); the in-tree trainer knows the number right here
            import dataclasses
            densify = dataclasses.replace(densify, num_train_data=len(scene.train_indices))
    ev_pos = 0
    first, wall0 = 1, 0.0
    if loaded is not None:
        tr = loaded.trainer
        first, seed, ev_pos = int(tr["iteration"]) + 1, int(tr["seed"]), int(tr["ev_pos"])
        g.set_state(tr["generator_state"])
        order, history = [int(i) for i in tr["order"]], list(tr["history"])
        wall0, lr_scale = float(tr["wall_clock_time_seconds"]), float(tr["lr_scale"])
        if state is not None and loaded.densify_state is not None:
            state = loaded.densify_state
        C.restore_default_generators(tr, model.means.device)

    def save(it):
        import torch.distributed as dist
        from . import checkpoint as C
        if model.means.is_cuda:
            torch.cuda.synchronize()
        multi = dist.is_available() and dist.is_initialized()
        if not multi or dist.get_rank() == 0:
            C.save_checkpoint(checkpoint_path, model, optimizers, densify_state=state,
                              trainer=C.trainer_state(it, seed, g, order, ev_pos, history, wall0 + time.time() - t0,
                                                      lr_scale, ssim_lambda, densify, model.means.device))
        if multi:
            dist.barrier()

    for it in range(first, iterations + 1):
        if not order:
            order = [scene.train_indices[j] for j in torch.randperm(len(scene.train_indices), generator=g).tolist()]
        ids = [order.pop() for _ in range(min(max(batch_size, 1), len(order)))]

        def take(seq):                                     # a batch takes lists, a single view the items themselves
            if seq is None:
                return None
            return [seq[i] for i in ids] if batch_size > 1 else seq[ids[0]]
        h = train_step(model, optimizers, take(scene.cameras), take(images), ssim_lambda, gt_depth=take(depths),
                       depth_lambda=depth_lambda, depth_loss=depth_loss, depth_space=depth_space, gt_normal=take(normals),
                       **normal_kw)
        if use_mcmc:
            M.step_callback(model, optimizers, it, densify)
        elif densify is not None:
            from . import densify as D
            D.step_callback(model, optimizers, state, it, densify)
        if optimize_eval_cameras and scene.eval_indices and it % eval_camera_every == 0:
            e = scene.eval_indices[ev_pos % len(scene.eval_indices)]
            ev_pos += 1
            eval_camera_step(model, optimizers, scene.cameras[e], images[e], ssim_lambda)
        if log_every and it % log_every == 0:
            history.append({"step": it, **h})
        if checkpoint_path is not None and (it == iterations or (checkpoint_every and it % checkpoint_every == 0)):
            save(it)
    if model.means.is_cuda:
        torch.cuda.synchronize()
    wall = wall0 + time.time() - t0
    res = evaluate(model, scene.cameras, images, scene.eval_indices, batch_size=batch_size)
    return {"results": res, "wall_clock_time_seconds": wall, "history": history}
