"""3DGS-MCMC densification (Kheradmand et al. 2024, "3D Gaussian Splatting as Markov Chain Monte Carlo"; gsplat's
``MCMCStrategy``) — the fixed-budget alternative to densify.py's split / duplicate / cull schedule.

gsplat is not part of the reference tree; the rules below are recollected from gsplat 1.x (``strategy/mcmc.py``,
``strategy/ops.py``: ``relocate``, ``sample_add``, ``inject_noise_to_position``; ``relocation.cu``), like densify.py's
are from splatfacto:

  * every ``refine_every`` steps between ``refine_start_iter`` and ``refine_stop_iter``: DEAD Gaussians (opacity <=
    ``min_opacity``) are teleported onto live ones drawn with probability proportional to opacity; a Gaussian that now
    stands n times in one place gets opacity ``1 - (1 - o)^(1/n)`` and a scale shrunk so that the n copies render what
    the one rendered (``gs_mcmc_relocation``); then the model grows by ``grow_factor`` towards the hard cap ``cap_max``
    by appending copies drawn the same way.  N never shrinks and never exceeds ``cap_max``;
  * after EVERY optimizer step the means receive noise ``Sigma * z * gate(opacity) * noise_lr * lr_means``: transparent
    Gaussians explore, opaque ones stay (``gs_mcmc_inject_noise``, one launch, no host synchronisation);
  * no screen-space statistic: ``collect_densify_stats`` stays off, no ``xy_grad`` work runs in the backward;
  * the strategy relies on ``SplatfactoDeblurConfig.opacity_reg`` / ``scale_reg`` (upstream 0.01 each) to let
    Gaussians die.  They give every row a gradient, so with ``optimizer="selective_adam"`` the "touched" mask is dense;
    "visible" is the mask that makes sense with MCMC.

On GPU tensors the two HIP kernels are the only route.  The torch restatements below serve CPU tensors (the host-logic
tests, as ``train_step.SelectiveAdam`` serves ``gs_adam_step_rows``) and the ``GSD_TORCH_TRAIN`` A/B switch; the torch
noise draws its normals from ``torch.randn`` under a generator seeded by (seed, step), not from the kernel's Philox
stream.  Data parallel: every decision is a function of the replicated parameters and of (seed, step), so the ranks
stay bit-identical without a broadcast.  ``torch.multinomial`` limits the sampled population to 2^24 rows.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

from .densify import _quat_to_rotmat, _swap_parameter
from .model import SplatfactoDeblurModel

MAX_RATIO = 51            # csrc/mcmc_math.h kMaxRatio


@dataclass
class MCMCConfig:
    cap_max: int = 1_000_000
    noise_lr: float = 5e5
    refine_start_iter: int = 500
    refine_stop_iter: int = 25_000
    refine_every: int = 100
    min_opacity: float = 0.005
    grow_factor: float = 1.25
    seed: int = 0


# --------------------------------------------------------------------------- #
# the two kernels: HIP on GPU tensors, torch otherwise
# --------------------------------------------------------------------------- #
def _use_hip(t: Tensor) -> bool:
    from .train_step import TORCH_TRAIN
    return t.is_cuda and not TORCH_TRAIN


def _f32c(t: Tensor, name: str) -> Tensor:
    if not t.is_cuda:
        raise ValueError(f"{name} must be a CUDA(HIP) tensor: the HIP path has no CPU fallback")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous float32")
    return t


def inject_noise_hip(means: Tensor, log_scales: Tensor, quats: Tensor, opacity_logits: Tensor, scaler: float,
                     seed: int, step: int, noise_in: Optional[Tensor] = None,
                     noise_out: Optional[Tensor] = None) -> None:
    """gs_mcmc_inject_noise: means [N,3] += Sigma (z gate scaler) in place; one launch on the current stream"""
    from . import _lib
    N = int(means.shape[0])
    for t, name, shape in ((means, "means", (N, 3)), (log_scales, "log_scales", (N, 3)), (quats, "quats", (N, 4)),
                           (noise_in, "noise_in", (N, 3)), (noise_out, "noise_out", (N, 3))):
        if t is not None:
            _f32c(t, name)
            if tuple(t.shape) != shape or t.device != means.device:
                raise ValueError(f"{name} must be {shape} on the means' device")
    _f32c(opacity_logits, "opacity_logits")
    if opacity_logits.numel() != N or opacity_logits.device != means.device:
        raise ValueError("opacity_logits must hold N values on the means' device")
    if N == 0:
        return
    L = _lib.load()
    vp = ctypes.c_void_p
    with torch.cuda.device(means.device):
        _lib.check(L.gs_mcmc_inject_noise(N, vp(means.data_ptr()), vp(log_scales.data_ptr()), vp(quats.data_ptr()),
                                          vp(opacity_logits.data_ptr()), float(scaler), int(seed), int(step),
                                          vp(noise_in.data_ptr() if noise_in is not None else None),
                                          vp(noise_out.data_ptr() if noise_out is not None else None),
                                          vp(torch.cuda.current_stream().cuda_stream)), "mcmc_inject_noise")


def relocation_hip(opacities: Tensor, scales: Tensor, ratios: Tensor) -> Tuple[Tensor, Tensor]:
    """gs_mcmc_relocation: opacities [M], scales [M,3] (linear units), ratios int32 [M] -> (new opacities, new scales)"""
    from . import _lib
    M = int(opacities.numel())
    _f32c(opacities, "opacities")
    _f32c(scales, "scales")
    if tuple(scales.shape) != (M, 3) or ratios.numel() != M or ratios.dtype != torch.int32 or not ratios.is_cuda \
            or not ratios.is_contiguous():
        raise ValueError("scales must be [M,3] and ratios contiguous int32 [M] on the GPU")
    new_o, new_s = torch.empty_like(opacities), torch.empty_like(scales)
    if M == 0:
        return new_o, new_s
    L = _lib.load()
    vp = ctypes.c_void_p
    with torch.cuda.device(opacities.device):
        _lib.check(L.gs_mcmc_relocation(M, vp(opacities.data_ptr()), vp(scales.data_ptr()), vp(ratios.data_ptr()),
                                        vp(new_o.data_ptr()), vp(new_s.data_ptr()),
                                        vp(torch.cuda.current_stream().cuda_stream)), "mcmc_relocation")
    return new_o, new_s


def _noise_generator(device, seed: int, step: int) -> torch.Generator:
    gen = torch.Generator(device=device)
    gen.manual_seed((int(seed) * 1000003 + int(step)) % (2 ** 63))
    return gen


@torch.no_grad()
def inject_noise_torch(means: Tensor, log_scales: Tensor, quats: Tensor, opacity_logits: Tensor, scaler: float,
                       seed: int, step: int, noise_in: Optional[Tensor] = None,
                       noise_out: Optional[Tensor] = None) -> None:
    """the noise kernel's math as torch ops (CPU tensors, A/B); normals from torch.randn seeded by (seed, step)"""
    if noise_in is None:
        noise_in = torch.randn(means.shape, device=means.device, dtype=means.dtype,
                               generator=_noise_generator(means.device, seed, step))
    if noise_out is not None:
        noise_out.copy_(noise_in)
    o = torch.sigmoid(opacity_logits.reshape(-1, 1))
    gate = torch.sigmoid(-100.0 * (o - 0.005))               # 1 / (1 + exp(100 (o - 0.005)))
    R = _quat_to_rotmat(quats)
    s = torch.exp(log_scales)
    cov = torch.bmm(R * (s * s)[:, None, :], R.transpose(1, 2))
    means.add_(torch.bmm(cov, (noise_in * gate * scaler)[..., None]).squeeze(-1))


@torch.no_grad()
def relocation_torch(opacities: Tensor, scales: Tensor, ratios: Tensor) -> Tuple[Tensor, Tensor]:
    """the relocation kernel's math as torch ops, summed in float64 like the kernel"""
    n = ratios.to(torch.int64).clamp(1, MAX_RATIO)
    o = opacities.double()
    nd = n.double()
    op = -torch.expm1(torch.log1p(-o) / nd)
    D = torch.zeros_like(o)
    binom = torch.ones_like(o)
    pw = torch.ones_like(o)
    for k in range(int(n.max()) if n.numel() else 0):
        binom = binom * (nd - k) / (k + 1)                   # C(n, k+1); 0 from k = n on
        pw = pw * op
        D = D + (-1.0) ** k * binom * pw / (k + 1) ** 0.5
    coeff = torch.where(D > 0, o / D, torch.ones_like(D))
    return op.to(opacities.dtype), (scales.double() * coeff[:, None]).to(scales.dtype)


def _relocation(opacities: Tensor, scales: Tensor, ratios: Tensor) -> Tuple[Tensor, Tensor]:
    if _use_hip(opacities):
        return relocation_hip(opacities.contiguous(), scales.contiguous(), ratios.to(torch.int32).contiguous())
    return relocation_torch(opacities, scales, ratios)


# --------------------------------------------------------------------------- #
# the strategy
# --------------------------------------------------------------------------- #
def _sample_and_correct(model: SplatfactoDeblurModel, probs: Tensor, population: Optional[Tensor], n: int, step: int,
                        cfg: MCMCConfig, salt: int) -> Tensor:
    """draw n rows with probability proportional to `probs` (over `population`, row ids, or over all rows), and write
    the corrected opacity / scale of the now multiply-occupied places into them; returns the drawn row ids [n]"""
    dev = model.means.device
    gen = torch.Generator(device=dev)
    gen.manual_seed((cfg.seed * 1000003 + step) * 2 + salt)
    drawn = torch.multinomial(probs, n, replacement=True, generator=gen)
    sampled = drawn if population is None else population[drawn]
    ratios = torch.bincount(sampled, minlength=model.num_points)[sampled] + 1
    o = torch.sigmoid(model.opacities.data.reshape(-1)[sampled])
    s = torch.exp(model.scales.data[sampled])
    new_o, new_s = _relocation(o, s, ratios.to(torch.int32))
    new_o = torch.clamp(new_o, min=cfg.min_opacity, max=1.0 - 1e-7)
    model.opacities.data[sampled] = torch.logit(new_o).reshape(-1, 1)
    model.scales.data[sampled] = torch.log(new_s)
    return sampled


@torch.no_grad()
def relocate(model: SplatfactoDeblurModel, optimizers: Dict[str, torch.optim.Optimizer], step: int,
             cfg: MCMCConfig) -> Dict[str, int]:
    """Teleport every dead Gaussian (sigmoid(opacity) <= min_opacity) onto a live one drawn by opacity; the live one and
    its new copies share the corrected opacity / scale, and the live one's Adam moments restart from zero (upstream
    resets the moments of the sampled rows, not of the rows that moved).  N is unchanged."""
    N = model.num_points
    opac = torch.sigmoid(model.opacities.data.reshape(-1))
    dead = opac <= cfg.min_opacity
    n_dead = int(dead.sum())
    if n_dead == 0 or n_dead == N:
        return {"relocated": 0, "dead": n_dead, "before": N, "after": N}
    dead_idx = dead.nonzero().reshape(-1)
    alive_idx = (~dead).nonzero().reshape(-1)
    sampled = _sample_and_correct(model, opac[alive_idx], alive_idx, n_dead, step, cfg, salt=0)
    for name, p in model.gauss_params().items():
        p.data[dead_idx] = p.data[sampled]
        opt = optimizers.get(name)
        st = opt.state.get(p) if opt is not None else None
        if st:
            for key in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
                if key in st:
                    st[key][sampled] = 0
    return {"relocated": n_dead, "dead": n_dead, "before": N, "after": N}


@torch.no_grad()
def add_new(model: SplatfactoDeblurModel, optimizers: Dict[str, torch.optim.Optimizer], step: int,
            cfg: MCMCConfig) -> Dict[str, int]:
    """Grow to min(cap_max, int(grow_factor * N)) by appending copies of rows drawn by opacity over ALL rows; the drawn
    rows and their copies share the corrected opacity / scale; the appended rows start with zero Adam moments."""
    N = model.num_points
    n_target = min(int(cfg.cap_max), int(cfg.grow_factor * N))
    n_new = max(0, n_target - N)
    if n_new == 0 or N == 0:
        return {"added": 0, "before": N, "after": N}
    opac = torch.sigmoid(model.opacities.data.reshape(-1))
    sampled = _sample_and_correct(model, opac, None, n_new, step, cfg, salt=1)
    for name, p in list(model.gauss_params().items()):
        _swap_parameter(model, optimizers, name, torch.cat([p.data, p.data[sampled]]), None, n_new)
    return {"added": n_new, "before": N, "after": model.num_points}


@torch.no_grad()
def inject_noise(model: SplatfactoDeblurModel, optimizers: Dict[str, torch.optim.Optimizer], step: int,
                 cfg: MCMCConfig) -> None:
    """means += Sigma z gate(opacity) * noise_lr * (the means optimizer's current learning rate); one kernel launch,
    nothing is read back"""
    opt = optimizers.get("means")
    if opt is None:
        raise ValueError("inject_noise needs the means optimizer (its learning rate scales the noise)")
    scaler = float(cfg.noise_lr) * float(opt.param_groups[0]["lr"])
    fn = inject_noise_hip if _use_hip(model.means) else inject_noise_torch
    fn(model.means.data, model.scales.data, model.quats.data, model.opacities.data, scaler, cfg.seed, step)


def step_callback(model: SplatfactoDeblurModel, optimizers: Dict[str, torch.optim.Optimizer], step: int,
                  cfg: MCMCConfig, group=None) -> Optional[Dict[str, int]]:
    """Call once per training step AFTER the optimizer step: relocate + add on schedule (refine_start_iter < step <
    refine_stop_iter, step % refine_every == 0), then the position noise of EVERY step.  `group`: accepted for symmetry
    with densify.step_callback — no statistic is exchanged, the ranks decide alike from their replicated parameters."""
    result = None
    if cfg.refine_start_iter < step < cfg.refine_stop_iter and step % cfg.refine_every == 0:
        r = relocate(model, optimizers, step, cfg)
        a = add_new(model, optimizers, step, cfg)
        result = {"relocated": r["relocated"], "added": a["added"], "before": r["before"], "after": a["after"]}
        # N and the opacity distribution changed: the row-sparse gradient exchange must not size its payload from old
        # counts
        from . import dp
        dp.notify_regime_change()
    inject_noise(model, optimizers, step, cfg)
    return result
