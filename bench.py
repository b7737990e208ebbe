#!/usr/bin/env python
"""bench.py — fwd+bwd rasterize throughput of the hot path on MI355X.

Contract (driver): `python bench.py --gpus N --steps K --warmup W`; for N>1 it is launched under
torch.distributed.run with one rank per GPU (RCCL).  W untimed warm-up steps, then EXACTLY K timed
steps bracketed by barrier + synchronize; MAX over ranks; rank 0 prints ONE JSON line.

A "step" = one forward + backward of the full path for one camera view per rank:
  SE(3) sub-pose viewmats -> fused projection of all Gaussians under S sub-poses (+SH, opacity)
  -> depth pre-sort, tile emission, stable tile sort, bin edges -> per-pixel composite of the S
  sample images -> gamma-space average -> dL/d(image) -> reverse-order rasterize backward ->
  projection/SH backward to all Gaussian parameters, viewmat and velocity gradients
  (+ for N>1: one all-reduce of the flattened Gaussian gradients).
Workload = BASELINE.json's metric configuration: 1M Gaussians, 1920x1080, 5 motion-blur sub-poses,
SH degree 3, seeded synthetic scene of SURVEY.md §8d; inputs resident in HBM before timing.
Weak scaling: every rank renders its own view of the same (replicated) Gaussians.

A plain run only sets up, warms up, times the K steps and prints the line (metric, value, unit, ms_per_step, ...).
`--full` adds what the headline does not need: the per-stage table and host-stall check, the roofline, the view sweep,
the secondary scene with its training step, the CPU baseline and the per-rank diagnostics.
`--dump-outputs DIR` writes what the last timed step computed (image, gradients of every input; a fixed seeded sample of
the per-Gaussian rows and their sums over all rows) as DIR/<name>.npy, so that two builds can be compared output for
output on identical inputs.
"""
import argparse
import json
import math
import os
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

DOMINANT_STAGE = "raster_bwd"   # the kernel the roofline is quoted on (checked against the stage table)
HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak (MI355X_MICROARCH.md: 8.0 TB/s; ~6.3 TB/s achievable)


def _counters_current(tj, build, kname=None) -> bool:
    """profiles/traffic.json was measured on the kernel sources that are on disk now (csrc + flags; a file from before
    round 4's kernel_source_hash is gated on the hash of the whole library source, public header included) — or, for the
    counters of ONE kernel, on that kernel's machine code: the file's kernel_isa_hash[kname] equals the hash of the ISA
    the in-tree library was built with (_build.stored_isa_hashes; a change elsewhere in csrc/ leaves it valid)"""
    if "kernel_source_hash" in tj:
        if tj["kernel_source_hash"] == build.kernel_source_hash():
            return True
        want = (tj.get("kernel_isa_hash") or {}).get(kname) if kname else None
        return bool(want) and build.stored_isa_hashes().get(kname) == want
    return tj.get("lib_source_hash") == build.source_hash()


def make_scene(n, W, H, seed=1234, profile="survey"):
    from gsdeblur_amd import data
    return data.synthetic_scene(n, W, H, sh_degree=3, seed=seed, profile=profile)


class Workload:
    """One camera view per rank of a replicated scene: parameters, view, fixed dL/d(image), and the step."""

    def __init__(self, gs, dev, rank, world, N, W, H, S, R, profile, allreduce, force_exchange=False, autograd=False,
                 motion="se3"):
        self.motion = motion
        self.gs, self.world, self.allreduce, self.force_exchange = gs, world, allreduce, force_exchange
        self.autograd = autograd
        self.S, self.R, self.H, self.W = S, R, H, W
        sc = self.sc = make_scene(N, W, H, profile=profile)
        names = ["means", "log_scales", "quats", "opacity_logits", "sh"]
        self.params = {k: sc[k].to(dev).requires_grad_(True) for k in names}
        # every rank renders its own view: rotate / shift the camera and vary the velocity per rank
        g = torch.Generator().manual_seed(1000 + rank)
        self.lin = (sc["lin_vel"] * (1.0 + 0.1 * rank)).to(dev).requires_grad_(True)
        self.ang = (sc["ang_vel"] * (1.0 + 0.1 * rank)).to(dev).requires_grad_(True)
        # rank r looks at the scene from a pose moved by (0.05 r, 0, 0) m and rotated by 0.01 r rad about y
        with torch.no_grad():
            V0 = gs.subpose_viewmats(torch.eye(4, device=dev), torch.tensor([0.05 * rank, 0.0, 0.0], device=dev),
                                     torch.tensor([0.0, 0.01 * rank, 0.0], device=dev), torch.ones(1, device=dev))[0]
        self.viewmat = V0.clone().requires_grad_(True)
        times, _, _ = gs.subpose_schedule(S, sc["exposure_time"], R, sc["rolling_shutter_time"])
        self.times_t = torch.tensor(times, device=dev)
        self.wt = torch.rand(H, W, 3, generator=g).to(dev)        # dL/d(image): fixed random weights
        self.bg = torch.zeros(3, device=dev)
        self.all_params = list(self.params.values())
        self.exchange_events = []
        # this scene's frame-to-frame hints (adaptive slice budget, arena estimate): owned by the workload, as
        # SplatfactoDeblurModel owns its own — the headline and the secondary scene have the same shape
        self.hints = gs.ops.FrameHints()
        self.view_key = None
        self.last_out = None            # the rendered image [H,W,3] of the last step (--dump-outputs)

    def warm_until_settled(self, at_least: int, at_most: int = 16) -> int:
        """untimed frames until the adaptive slice budget and the arena have converged (two consecutive frames with the
        same slice count, the budget the next frame will use, and no arena retry) -> frames run"""
        k = 0
        if self.world > 1:
            # a step holds a collective: every rank must run the SAME number of frames, and "settled" is a per-rank fact
            # (each rank renders its own view) — a fixed count, longer than the budget's three doublings
            for _ in range(max(at_least, 6)):
                self.step()
                k += 1
            return k
        while k < at_least or (k < at_most and not self.hints.settled):
            self.step()
            k += 1
        return k

    def step(self):
        gs, sc, params = self.gs, self.sc, self.params
        for p in self.all_params + [self.lin, self.ang, self.viewmat]:
            p.grad = None
        if not self.autograd:
            # default: forward + backward of the frame as ONE host call (gsdeblur_amd.step.render_step: the same C-ABI
            # calls as the autograd node below, issued back to back, no autograd engine between the two compositors);
            # fixed d loss / d image = wt; every Gaussian parameter, the view matrix and the velocities get their gradient
            out, g, _ = gs.render_step(params["means"], params["log_scales"], params["quats"], params["opacity_logits"],
                                       params["sh"], self.viewmat, self.lin, self.ang, self.times_t, self.bg, self.S,
                                       self.R, sc["fx"], sc["fy"], sc["cx"], sc["cy"], self.H, self.W, self.wt, gamma=2.2,
                                       min_rgb_level=10.0, sh_degree=3, antialiased=True, raw_params=True,
                                       motion_model="se3" if self.motion == "se3" else "pixel_velocity",
                                       shared_list=self.motion == "pixel_velocity_shared", hints=self.frame_hints())
            for k, name in (("means", "means"), ("log_scales", "scales"), ("quats", "quats"),
                            ("opacity_logits", "opacities"), ("sh", "sh")):
                params[k].grad = g[name]
            self.viewmat.grad, self.lin.grad, self.ang.grad = g["viewmat"], g["lin_vel"], g["ang_vel"]
            if self.world > 1 or self.force_exchange:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                gs.dp.allreduce_gradients(self.all_params, mode=self.allreduce, force=self.force_exchange)
                b.record()
                self.exchange_events.append((a, b))
            self.last_out = out
            return out
        vms = gs.subpose_viewmats(self.viewmat, self.lin, self.ang, self.times_t)
        # the raw parameters (log-scales, opacity logits) go to the kernels as they are: activations and their backward
        # run inside the projection (no torch launches between the HIP stages)
        out, _, _ = gs.render_combined(params["means"], params["log_scales"], params["quats"],
                                       params["opacity_logits"], params["sh"], vms, self.bg, self.S,
                                       self.R, sc["fx"], sc["fy"], sc["cx"], sc["cy"], self.H, self.W, gamma=2.2,
                                       min_rgb_level=10.0, sh_degree=3, antialiased=True,
                                       return_alpha=False, raw_params=True, hints=self.frame_hints())   # the loss reads RGB only
        # fixed d loss / d image = wt (the loss (out * wt).sum() without its two launches: the step times the renderer's
        # forward + backward to every parameter, not a reduction)
        out.backward(self.wt)
        loss = out
        if self.world > 1 or self.force_exchange:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            gs.dp.allreduce_gradients(self.all_params, mode=self.allreduce, force=self.force_exchange)
            b.record()
            self.exchange_events.append((a, b))
        self.last_out = out
        return loss

    def sweep_views(self, n_views: int):
        """n_views distinct cameras around this workload's own: an orbit of yaw / pitch / position about the scene
        (amplitudes chosen so that most views stay inside the populated frustum slab and a few look past its edge), each
        with its own velocity scale and sign — the camera batch a training loop cycles through (/root/reference/train.py:
        115-116 -> ns-train: datamanager.next_train hands the model a DIFFERENT camera every iteration)"""
        gs, dev = self.gs, self.viewmat.device
        views = []
        with torch.no_grad():
            base = self.viewmat.detach().clone()
            for v in range(n_views):
                ph = 2.0 * math.pi * v / n_views
                shift = torch.tensor([0.10 * math.cos(ph), 0.06 * math.sin(ph), 0.05 * (v % 3)], device=dev)
                rot = torch.tensor([0.06 * math.cos(ph), 0.10 * math.sin(ph), 0.02 * ((v % 4) - 1.5)], device=dev)
                V = gs.subpose_viewmats(base, shift, rot, torch.ones(1, device=dev))[0]
                k = (1.0 + 0.1 * (v % 5)) * (-1.0 if v % 2 else 1.0)
                views.append((V.clone(), (self.sc["lin_vel"] * k).to(dev), (self.sc["ang_vel"] * k).to(dev)))
        return views

    def set_view(self, view, key=None):
        """key: the camera's index — its frames then go through hints.view(key), the camera's own memory inside the
        scene's FrameHints (None: the scene-level memory, as for the fixed headline view)"""
        V, lin, ang = view
        self.view_key = key
        self.viewmat = V.clone().requires_grad_(True)
        self.lin = lin.clone().requires_grad_(True)
        self.ang = ang.clone().requires_grad_(True)

    def frame_hints(self):
        return self.hints if self.view_key is None else self.hints.view(self.view_key)

    def rows_with_gradient(self):
        g = self.params["means"].grad
        return int((g != 0).any(dim=1).sum()) if g is not None else 0


def view_sweep(wl, ops, n_views=16, cycles=4, fixed_frames=6, per_camera=True, fixed=None):
    """A training-shaped sequence: n_views distinct cameras cycled through ONE FrameHints — the
    way SplatfactoDeblurModel owns one for all its cameras — against every view's own fixed-view time (the same view
    rendered back to back through a private FrameHints, which is what the headline measures).  per_camera: every camera's
    frames go through hints.view(camera index), its own memory inside that one FrameHints (what the Model does with
    camera.metadata['cam_idx']); False: one last-frame memory for all cameras (rounds 1-5, and any caller that passes no
    camera key).  Reported, never `value`."""
    import statistics
    gs = wl.gs
    views = wl.sweep_views(n_views)
    saved = (wl.viewmat, wl.lin, wl.ang, wl.hints, wl.view_key)

    def timed_step():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        wl.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    if fixed is None:
        fixed = []
        for view in views:                                      # each view's own steady state
            wl.set_view(view)
            wl.hints = gs.ops.FrameHints()
            ms = [timed_step() for _ in range(fixed_frames)]
            fixed.append(statistics.median(ms[2:]))
    wl.hints = gs.ops.FrameHints()                           # ONE hints object for the whole sweep
    per_view = [[] for _ in views]
    decisions, mults, slices, select_state = [], [], [], []
    retries0 = 0
    for c in range(cycles):
        for i, view in enumerate(views):
            wl.set_view(view, i if per_camera else None)
            h = wl.frame_hints()
            decisions.append((bool(ops.LAZY_RECORDS and h.lazy_records()), bool(ops.DEPTH_SELECT and h.depth_select())))
            ms = timed_step()
            mults.append(wl.hints.mult)
            slices.append(len([v for v in ops.last_slice_intersects if int(v) > 0]))
            select_state.append(ops.last_depth_select)
            if c == 0:
                retries0 = wl.hints.arena_retries
            else:
                per_view[i].append(ms)
    retries_all = wl.hints.arena_retries
    overflows = wl.hints.select_overflows
    wl.viewmat, wl.lin, wl.ang, wl.hints, wl.view_key = saved
    flat = [m for v in per_view for m in v]
    ratio = [max(v) / f for v, f in zip(per_view, fixed)]
    ratio_med = [statistics.median(v) / f for v, f in zip(per_view, fixed)]
    # (decisions of the later cycles only: in the first one every camera is new)
    later = decisions[len(views):]
    flips = lambda seq: sum(1 for a, b in zip(seq, seq[1:]) if a != b)
    hist = []
    for m in mults:
        if not hist or hist[-1] != m:
            hist.append(m)
    return {"views": n_views, "cycles": cycles, "frames_timed": len(flat),
            "memory": "one per camera (hints.view(camera index)) inside the one FrameHints" if per_camera else
                      "one last-frame memory for all cameras",
            "ms_per_view": {"min": round(min(flat), 4), "median": round(statistics.median(flat), 4), "max": round(max(flat), 4)},
            "fixed_view_ms": {"min": round(min(fixed), 4), "median": round(statistics.median(fixed), 4), "max": round(max(fixed), 4)},
            # a view's slowest frame of the later cycles (and its median frame) over the MEDIAN of its own fixed-view frames
            "worst_view_over_its_fixed_time": round(max(ratio), 3),
            "frames_over_1p5x_their_fixed_time": sum(1 for v, f in zip(per_view, fixed) for m in v if m > 1.5 * f),
            "worst_view_median_over_its_fixed_time": round(max(ratio_med), 3),
            "median_view_over_its_fixed_time": round(statistics.median(ratio), 3),
            "slices_per_frame": {"min": min(slices), "max": max(slices)},
            "lazy_eager_flips": flips([d[0] for d in decisions]), "selection_flips": flips([d[1] for d in decisions]),
            "selection_misses": sum(1 for s_ in select_state if s_ == 2),
            "selection_misses_after_first_cycle": sum(1 for s_ in select_state[len(views):] if s_ == 2),
            "frames_selecting_after_first_cycle": sum(1 for d in later if d[1]),
            "selection_outgrew_its_promised_size": overflows,
            "budget_multiplier_history": hist, "arena_retries_first_cycle": retries0,
            "arena_retries_later_cycles": retries_all - retries0,
            "_fixed": fixed,
            "note": "wall clock per frame (synchronize around every step: includes launch latency the back-to-back "
                    "headline loop hides); first cycle untimed; never part of `value`"}


def _import_oracle():
    """The CPU oracle is test infrastructure: ONLY the cpu_baseline leg below loads it."""
    sys.path.insert(0, str(ROOT / "oracle"))
    import gs_oracle
    return gs_oracle


def cpu_baseline():
    """The CPU oracle (kind 'port': this repo's own restatement — gsplat's _torch_impl is not in the
    reference tree) timed on BASELINE.json config 1: 5k Gaussians, 256x256, 1 sub-pose, fwd+bwd, fp32.
    The same scene is then rendered through the HIP path and compared (SURVEY §8d "PSNR vs oracle render")."""
    O = _import_oracle()
    W = H = 256
    n = 5000
    sc = O.synthetic_scene(n, W, H, seed=1234, scale_mult=4.0)
    cfg = O.RenderConfig(H, W, sc["fx"], sc["fy"], sc["cx"], sc["cy"], blur_samples=1, rs_bands=1)
    # threads: torch's default, capped by the CPU affinity mask and 16 (os.cpu_count() ignores cgroup
    # limits; oversubscribing tiny per-tile tensor ops makes the baseline pathologically slow)
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    cores = max(1, min(torch.get_num_threads(), avail, 16))
    torch.set_num_threads(cores)
    names = ["means", "log_scales", "quats", "opacity_logits", "sh"]

    def one():
        p = {k: sc[k].clone().requires_grad_(True) for k in names}
        out, _ = O.render(cfg, p["means"], p["log_scales"].exp(), p["quats"], torch.sigmoid(p["opacity_logits"]),
                          p["sh"], sc["viewmat"], sc["lin_vel"], sc["ang_vel"])
        out.mean().backward()

    one()
    t0 = time.perf_counter()
    reps = 0
    while True:
        one()
        reps += 1
        if time.perf_counter() - t0 > 10.0 or reps >= 20:
            break
    dt = (time.perf_counter() - t0) / reps
    res = {"value": round(W * H / 1e6 / dt, 5), "unit": "MPix/s", "cores": cores, "kind": "port",
           "sample": f"own CPU oracle (torch fp32, vectorised per tile), BASELINE config 1: 5k Gaussians 256x256 "
                     f"1 sub-pose (SURVEY 8d scene with scale_mult=4.0 so that 5k Gaussians cover the frame), "
                     f"fwd+bwd, mean of {reps} runs = {dt * 1e3:.0f} ms"}
    # parity of the measured path on the baseline's own workload: HIP render vs the oracle's render
    import gsdeblur_amd as gs
    with torch.no_grad():
        ref, _ = O.render(cfg, sc["means"], sc["log_scales"].exp(), sc["quats"], torch.sigmoid(sc["opacity_logits"]),
                          sc["sh"], sc["viewmat"], sc["lin_vel"], sc["ang_vel"])
        dev = torch.device("cuda", torch.cuda.current_device())
        vms = sc["viewmat"].to(dev)[None]
        samples, _, _ = gs.render_subposes(sc["means"].to(dev), sc["log_scales"].exp().to(dev), sc["quats"].to(dev),
                                           torch.sigmoid(sc["opacity_logits"]).to(dev), sc["sh"].to(dev), vms, None,
                                           1, 1, sc["fx"], sc["fy"], sc["cx"], sc["cy"], H, W, sh_degree=3)
        got = gs.combine_samples(samples, cfg.gamma, cfg.min_rgb_level).cpu()
    err = (got - ref).abs()
    mse = float((err.double() ** 2).mean())
    res["parity_vs_oracle"] = {"psnr_db": round(10.0 * math.log10(1.0 / max(mse, 1e-30)), 2),
                               "max_abs": float(err.max()), "pixels_over_1e-3": int((err.max(dim=-1).values > 1e-3).sum())}
    return res


def guarded_cpu_baseline(limit_s: int = 150):
    """Never let the (reported-only) CPU leg cost the GPU line: hard time limit via SIGALRM."""
    import signal

    class _Timeout(Exception):
        pass

    def _raise(*_):
        raise _Timeout()

    old = signal.signal(signal.SIGALRM, _raise)
    signal.alarm(limit_s)
    try:
        return cpu_baseline()
    except _Timeout:
        return {"value": None, "unit": "MPix/s", "cores": None, "kind": "port",
                "sample": f"own CPU oracle did not finish 5k Gaussians 256x256 fwd+bwd within {limit_s} s"}
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


def train_step_timing(gs, dev, sc, N, W, H, S, steps=5):
    """One full training iteration on the secondary scene through the model surface: render (HIP) -> image loss
    (0.8 L1 + 0.2 (1 - SSIM)) -> backward -> Adam on the six Gaussian groups; once with the HIP loss / optimizer kernels
    (csrc/train.hip), once with the torch formulations they replace (conv2d SSIM + autograd, six torch.optim.Adam)."""
    import time as _t
    cfg = gs.SplatfactoDeblurConfig(blur_samples=S, rolling_shutter_compensation=False, gamma=2.2, min_rgb_level=10.0)
    c2w = torch.eye(4)[:3].clone()
    c2w[:, 1] *= -1
    c2w[:, 2] *= -1
    cam = gs.Camera(c2w, sc["fx"], sc["fy"], sc["cx"], sc["cy"], W, H,
                    metadata=dict(cam_idx=0, camera_linear_velocity=[float(v) for v in sc["lin_vel"] * torch.tensor([1., -1., -1.])],
                                  camera_angular_velocity=[float(v) for v in sc["ang_vel"] * torch.tensor([1., -1., -1.])],
                                  exposure_time=sc["exposure_time"], rolling_shutter_time=0.0))
    target = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(7)).to(dev)
    res = {}
    for tag, fused in (("hip_loss_and_adam", True), ("torch_loss_and_adam", False)):
        model = gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev)
        opts = gs.training.make_optimizers(model, fused=fused)

        def one():
            if fused:
                gs.training.train_step(model, opts, cam, target, 0.2)
                return
            model.train()
            for o in opts.values():
                o.zero_grad(set_to_none=True)
            out = model.get_outputs(cam)
            gs.training.image_loss_torch(out["rgb"], target, 0.2).backward()
            for o in opts.values():
                o.step()
            model.step += 1
        for _ in range(2):
            one()
        torch.cuda.synchronize()
        t0 = _t.perf_counter()
        for _ in range(steps):
            one()
        torch.cuda.synchronize()
        res[tag + "_ms"] = round((_t.perf_counter() - t0) / steps * 1e3, 3)
        del model, opts
        torch.cuda.empty_cache()
    res["note"] = ("full iteration on the secondary scene: render + loss + backward + optimizer step; train_step also "
                   "reads the loss back for logging")
    return res


DUMP_GAUSSIAN_ROWS = 1 << 16     # per-Gaussian gradients: a fixed sample of this many rows (SH alone is 192 MB at 1M)
DUMP_PIXELS = 1 << 21            # the image is written whole up to this many pixels (1920x1080 fits), else sampled


def _fixed_rows(n: int, k: int, seed: int):
    """sorted indices of a seeded sample of k of n rows (all rows when n <= k): the same for every run and every build"""
    if n <= k:
        return None
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:k].sort().values


def _index_array(idx):
    """row indices as floats: float32 holds every integer below 2^24 exactly, float64 the rest"""
    return idx.float() if int(idx.max()) < (1 << 24) else idx.double()


def dump_outputs(wl, out_dir) -> dict:
    """What the last timed step handed its caller — the image and the gradients of every input (raw parameters, view
    matrix, velocities) — as out_dir/<name>.npy in float32 (at most ~50 MB in all).  Arrays larger than the caps above are
    reduced to a fixed, seeded sample of their rows, and the sampled row indices are written beside them.  Every
    per-Gaussian gradient also gets grad_<name>_all_rows (float64): its column sums and sums of magnitudes over ALL rows,
    so that a row outside the sample still counts -> {name: shape}"""
    import numpy as np
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    arrays = {}
    img = wl.last_out.detach()                                  # [H,W,3]
    pix = _fixed_rows(img.shape[0] * img.shape[1], DUMP_PIXELS, seed=1)
    if pix is None:
        arrays["image"] = img
    else:                                                       # [DUMP_PIXELS,3] of the flattened image
        arrays["image"] = img.reshape(-1, img.shape[-1])[pix.to(img.device)]
        arrays["image_pixel_rows"] = _index_array(pix)
    rows = _fixed_rows(wl.params["means"].shape[0], DUMP_GAUSSIAN_ROWS, seed=2)
    for k, p in wl.params.items():
        g = (p.grad if p.grad is not None else torch.zeros_like(p)).detach()
        arrays["grad_" + k] = g if rows is None else g[rows.to(g.device)]
        arrays[f"grad_{k}_all_rows"] = torch.stack([g.double().sum(dim=0), g.double().abs().sum(dim=0)])
    if rows is not None:
        arrays["gaussian_rows"] = _index_array(rows)
    for k, p in (("viewmat", wl.viewmat), ("lin_vel", wl.lin), ("ang_vel", wl.ang)):
        arrays["grad_" + k] = p.grad.detach() if p.grad is not None else torch.zeros_like(p)
    shapes = {}
    for name, a in arrays.items():
        a = a.cpu()
        a = a if a.dtype == torch.float64 else a.float()
        np.save(out_dir / f"{name}.npy", a.numpy())
        shapes[name] = list(a.shape)
    return shapes


def launcher_argv(gpus: int, argv, environ, port=None):
    """`python bench.py --gpus N` without a launcher becomes the launcher: -> the torch.distributed.run command line
    (one rank per GPU over RCCL, rendezvous on 127.0.0.1), or None when this process already is a rank / N == 1."""
    if gpus <= 1 or "WORLD_SIZE" in environ:
        return None
    if port is None:
        import socket
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={gpus}",
            "--master-addr", "127.0.0.1", "--master-port", str(port), str(Path(__file__).resolve())] + list(argv)


def check_world(gpus: int, world: int) -> None:
    if world != gpus:
        raise SystemExit(f"bench.py --gpus {gpus} launched with WORLD_SIZE={world}: they must agree")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--subposes", type=int, default=5, help="motion-blur samples S")
    ap.add_argument("--rs-bands", type=int, default=1, help="rolling-shutter row bands R")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: per-stage table, host-stall check and retries, "
                         "roofline, view sweep, secondary scene (with its training step), CPU baseline, per-rank "
                         "diagnostics.  Without it a run sets up, warms up, times the K steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed (image, gradients of every input; a "
                         "fixed seeded sample of the per-Gaussian rows) as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(--full) skip the CPU oracle baseline")
    ap.add_argument("--allreduce", default="sparse", choices=["sparse", "allreduce", "rs_ag"],
                    help="DP gradient exchange: row-sparse all-gather (default; dense fallback built in), "
                         "dense all-reduce, or reduce-scatter + all-gather")
    ap.add_argument("--no-secondary", action="store_true", help="(--full) skip the second (fitted-model-like) scene")
    ap.add_argument("--strict-stall", action="store_true",
                    help="implies --full; exit 3 when a host stall above 10 %% of the step survives three timing attempts "
                         "(always reported in `host_stall_check` with --full)")
    ap.add_argument("--view", type=int, default=None,
                    help="diagnostics: time camera K of the view sweep's 16 instead of the headline view (the line says so in "
                         "config.workload; never the headline)")
    ap.add_argument("--no-view-sweep", action="store_true",
                    help="(--full) skip the view sweep (16 cameras cycled through one FrameHints; reported beside the headline)")
    ap.add_argument("--autograd", action="store_true",
                    help="time the torch.autograd route (ops.render_combined + Tensor.backward) instead of the default "
                         "one-call forward + backward (gsdeblur_amd.render_step); same kernels, more host glue")
    ap.add_argument("--force-exchange", action="store_true",
                    help="run the DP gradient exchange over RCCL even at --gpus 1 (single-rank collectives: measures the "
                         "pack -> collective -> scatter chain's device cost as exchange_ms; the timed step includes it)")
    ap.add_argument("--motion", default="se3", choices=["se3", "pixel_velocity", "pixel_velocity_shared"],
                    help="how the sub-poses move the splats (BASELINE metric: se3 — every sub-pose re-projects); "
                         "pixel_velocity: one projection, S lists; pixel_velocity_shared: one projection, ONE list")
    ap.add_argument("--scene", default="survey", choices=["survey", "trained"],
                    help="scene profile of the timed workload (BASELINE metric: survey)")
    args = ap.parse_args()

    cmd = launcher_argv(args.gpus, sys.argv[1:], os.environ)
    if cmd is not None:
        import subprocess
        sys.exit(subprocess.call(cmd))

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    import torch.distributed as dist
    check_world(args.gpus, world)
    if torch.cuda.device_count() < (local_rank + 1):
        raise SystemExit(f"rank {rank}: no GPU {local_rank} on this node ({torch.cuda.device_count()} visible)")
    if world > 1 or args.force_exchange:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl", rank=rank, world_size=world)
        assert dist.get_world_size() == args.gpus
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)

    import gsdeblur_amd as gs
    from gsdeblur_amd import ops

    N, W, H, S, R = args.gaussians, args.width, args.height, args.subposes, args.rs_bands
    wl = Workload(gs, dev, rank, world, N, W, H, S, R, args.scene, args.allreduce, args.force_exchange, args.autograd,
                  args.motion)
    sc, params, step = wl.sc, wl.params, wl.step
    if args.view is not None:
        wl.set_view(wl.sweep_views(16)[args.view % 16])

    # W untimed warm-up frames, then further untimed ones until the scene's adaptive slice budget and arena have settled
    # (they normally have: the headline scene stops after its first slice) — no allocation inside the timed region
    warm_frames = wl.warm_until_settled(args.warmup)

    issue_trace = []

    def timed_region(w, k):
        """EXACTLY k steps between barrier + synchronize on both sides -> seconds (this rank)"""
        if world > 1:
            dist.barrier(device_ids=[local_rank])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        marks = [t0]
        for _ in range(k):
            w.step()
            marks.append(time.perf_counter())
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier(device_ids=[local_rank])
        t1 = time.perf_counter()
        # when the HOST finished issuing each step (a step ends in polled read-backs, so this tracks the device closely):
        # a stalled attempt shows WHICH step the host lost its time in
        issue_trace.clear()
        issue_trace.extend(round((b - a) * 1e3, 3) for a, b in zip(marks, marks[1:] + [t1]))
        return t1 - t0

    def stage_pass(w, k):
        """k extra (untimed) steps with HIP events around every stage -> {stage: [ms per launch]}"""
        ops.profiler = ops.StageProfiler()
        for _ in range(k):
            w.step()
        st = ops.profiler.summary_ms()
        ops.profiler = None
        return st

    # everything beside the headline (stage table, stall retries, roofline, sweep, secondary scene, CPU baseline, per-rank
    # diagnostics) runs with --full only; a plain run sets up, warms up, times the K steps and prints the line
    full = args.full or args.strict_stall
    # timed region (--full): HIP events only around the dominant kernel's launches (two event records per step) for the
    # roofline; every event record is a barrier packet in the queue, so the full per-stage table is taken in a separate,
    # untimed pass below.  A plain run times the steps without any profiler.
    ops.profiler = ops.StageProfiler(only={DOMINANT_STAGE}) if full else None
    dt = timed_region(wl, args.steps)
    timed_dom = ops.profiler.summary_ms() if full else {}
    ops.profiler = None
    exchange_ms = None
    if wl.exchange_events:
        torch.cuda.synchronize()
        ev = wl.exchange_events[-args.steps:]
        exchange_ms = sum(a.elapsed_time(b) for a, b in ev) / len(ev)
    # what the last timed step computed, before any further (untimed) step overwrites it
    dumped = dump_outputs(wl, args.dump_outputs) if args.dump_outputs and rank == 0 else None
    n_stage_steps = min(args.steps, 5)
    stages = stage_pass(wl, n_stage_steps) if full else None
    # host stall = step time no stage accounts for (the driver saw 86 ms/step on the secondary scene
    # against 8.7 ms of stages and the line said nothing).  Above 10 % of the step the K steps are timed again (every
    # attempt is reported); a stall that survives three attempts is flagged FAILED in the line (and fails the run with --strict-stall; world 1; with N > 1 the rank skew and the
    # exchange live in the same remainder and are reported per rank instead)
    def stall_of(ms, st, k, extra=0.0):
        return ms - sum(sum(v) for v in st.values()) / k - extra

    # `value` is the FIRST attempt, whatever the retries show (taking the last of 1-3 attempts selected
    # toward the fastest); the retries only tell whether a stall repeats
    attempts = [round(dt / args.steps * 1e3, 4)]
    first_issue_trace = list(issue_trace)
    while (full and world == 1 and len(attempts) < 3 and
           stall_of(attempts[-1], stages, n_stage_steps, exchange_ms or 0.0) > 0.10 * attempts[-1]):
        ops.profiler = ops.StageProfiler(only={DOMINANT_STAGE})
        dt_again = timed_region(wl, args.steps)
        ops.profiler = None
        attempts.append(round(dt_again / args.steps * 1e3, 4))
    stall_survives = full and stall_of(attempts[-1], stages, n_stage_steps, exchange_ms or 0.0) > 0.10 * attempts[-1]
    n_isect = ops.last_num_intersects
    slice_isects = list(ops.last_slice_intersects)
    slice_budget = wl.hints.slice_base()                    # (ops.SLICE_ADAPT: doubles after multi-slice frames)
    headline_hints = {"frames": wl.hints.frames, "arena_retries": wl.hints.arena_retries,
                      "arena_bytes": wl.hints.arena_bytes, "settled": wl.hints.settled, "warm_frames": warm_frames,
                      # lazy records: does this scene's next frame project without records, and on what grounds
                      "lazy_records": bool(args.motion == "se3" and (ops.LAZY_RECORDS == 2 or
                                                                       (ops.LAZY_RECORDS and wl.hints.lazy_records()))),
                      "box_share_of_issued_slices": None if wl.hints.box_share is None else round(wl.hints.box_share, 4),
                      # nearest-first selection: does the next frame rank only the pairs its first slice reaches, how many it
                      # promises the sort's tail passes, and how often a selection fell short / outgrew the promise
                      "depth_select": bool(ops.DEPTH_SELECT == 2 or (ops.DEPTH_SELECT and wl.hints.depth_select())),
                      "select_cap": wl.hints.select_cap, "select_misses": wl.hints.select_misses,
                      "select_overflows": wl.hints.select_overflows}
    rows_with_grad = wl.rows_with_gradient()
    sweep = None
    if full and world == 1 and not args.no_view_sweep and args.motion == "se3":
        sweep = view_sweep(wl, ops)
        # the same cameras through ONE last-frame memory (what rounds 1-5 did, and what a caller without camera keys gets)
        one = view_sweep(wl, ops, per_camera=False, fixed=sweep.pop("_fixed"))
        one.pop("_fixed", None)
        sweep["one_memory_for_all_cameras"] = {k: one[k] for k in (
            "ms_per_view", "worst_view_over_its_fixed_time", "worst_view_median_over_its_fixed_time",
            "median_view_over_its_fixed_time", "lazy_eager_flips", "selection_flips", "selection_misses",
            "frames_selecting_after_first_cycle", "budget_multiplier_history")}
    # second scene (reported beside the headline, never part of `value`): a fitted-model-like distribution in which
    # a large share of the Gaussians receives a gradient and the depth-sliced path needs several slices
    secondary = None
    if full and not args.no_secondary and args.scene == "survey":
        del wl, params, step
        torch.cuda.empty_cache()
        w2 = Workload(gs, dev, rank, world, N, W, H, S, R, "trained", args.allreduce, False, args.autograd, args.motion)
        warm2 = w2.warm_until_settled(2)
        k2 = max(3, min(args.steps, 10))
        dt2 = timed_region(w2, k2)
        if world > 1:
            tt = torch.tensor([dt2], device=dev, dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            dt2 = float(tt.item())
        st2 = stage_pass(w2, 3)
        attempts2 = [round(dt2 / k2 * 1e3, 4)]
        while world == 1 and len(attempts2) < 3 and stall_of(attempts2[-1], st2, 3) > 0.10 * attempts2[-1]:
            attempts2.append(round(timed_region(w2, k2) / k2 * 1e3, 4))
        stall2_survives = stall_of(attempts2[-1], st2, 3) > 0.10 * attempts2[-1]
        ms2 = dt2 / k2 * 1e3
        # the secondary scene's own roofline block: its dominant kernel on the same bytes formula
        st2m = {k: sum(v) / 3 for k, v in st2.items()}
        I2 = int(sum(ops.last_slice_intersects))
        npix2 = H * W
        bwd_bytes2 = 40 * I2 + S * 32 * npix2 + 36 * S * R * N
        sec_roofline = None
        if st2m.get("raster_bwd"):
            ach2 = bwd_bytes2 / (st2m["raster_bwd"] * 1e-3) / 1e9
            sec_roofline = {"bound": "hbm", "kernel": "raster_bwd_sload_kernel", "achieved": round(ach2, 2),
                            "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach2 / HBM_PEAK_GBS, 5),
                            "algorithmic_bytes_per_step": bwd_bytes2, "kernel_ms_per_step": round(st2m["raster_bwd"], 4),
                            "launches_per_step": len(st2["raster_bwd"]) / 3,
                            "kernel_time_source": "HIP events around every launch, 3 steps after the timed region"}
        train = train_step_timing(gs, dev, w2.sc, N, W, H, S) if world == 1 else None
        secondary = {
            "scene": "profile 'trained' (gsdeblur_amd.data.synthetic_scene): same seeded draws, world-space scale "
                     "0.006*z per Gaussian (constant ~7 px screen size), opacity logits ~ N(-3.3, 1.5^2)",
            "value": round(world * H * W / 1e6 / (ms2 / 1e3), 3), "unit": "MPix/s", "ms_per_step": round(ms2, 4),
            "steps": k2, "tile_intersections_per_step": ops.last_num_intersects,
            "tile_intersections_emitted": int(sum(ops.last_slice_intersects)),
            "depth_slices": list(ops.last_slice_intersects), "gaussians_with_gradient": w2.rows_with_gradient(),
            # ops.SLICE_ADAPT: the first slice's budget doubles (up to 8x) after a frame that issued two or more slices
            "slice_budget": w2.hints.slice_base(),
            "stage_ms": {k: round(sum(v) / 3, 4) for k, v in st2.items()},
            "host_stall_ms": round(stall_of(ms2, st2, 3), 4), "timing_attempts_ms": attempts2,
            "host_stall_survives_retries": bool(stall2_survives),
            "frame_hints": {"frames": w2.hints.frames, "arena_retries": w2.hints.arena_retries,
                            "arena_bytes": w2.hints.arena_bytes, "settled": w2.hints.settled, "warm_frames": warm2,
                            "lazy_records": bool(args.motion == "se3" and (ops.LAZY_RECORDS == 2 or
                                                                             (ops.LAZY_RECORDS and w2.hints.lazy_records()))),
                            "box_share_of_issued_slices": None if w2.hints.box_share is None else round(w2.hints.box_share, 4)},
            "roofline": sec_roofline, "train_step": train}
        del w2
        torch.cuda.empty_cache()
    # per-rank diagnostics (a SCALE record must explain itself: which rank was slow, what the exchange cost it)
    per_rank = rccl_version = None
    if full and (world > 1 or args.force_exchange):
        my_ms = dt / args.steps * 1e3
        info = {"rank": rank, "device": torch.cuda.get_device_name(dev), "ms_per_step": round(my_ms, 4),
                "exchange_ms": None if exchange_ms is None else round(exchange_ms, 4),
                # what no stage of THIS rank accounts for: launch gaps, read-back waits, skew against the slowest rank
                "host_stall_ms": round(stall_of(my_ms, stages, n_stage_steps, exchange_ms or 0.0), 4),
                "readback": gs.ops.readback_mode(),
                "gaussians_with_gradient": rows_with_grad}
        per_rank = [None] * world
        dist.all_gather_object(per_rank, info)
        try:
            rccl_version = ".".join(str(v) for v in torch.cuda.nccl.version())
        except Exception:
            rccl_version = None
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    ms_per_step = dt / args.steps * 1e3
    npix = H * W
    value = world * npix / 1e6 / (ms_per_step / 1e3)

    stall_check = None
    if rank == 0 and full:
        stage_ms = {k: round(sum(v) / n_stage_steps, 4) for k, v in stages.items()}   # per step (sum over slices)
        host_stall = stall_of(ms_per_step, stages, n_stage_steps, exchange_ms or 0.0)
        stall_check = "ok"
        if world == 1 and args.force_exchange:
            stall_check = "reported only (--force-exchange: the exchange's host glue lives in the same remainder)"
        elif world == 1:
            bad = [f"{tag} scene: {st:.3f} ms of a {ms:.3f} ms step no stage accounts for"
                   for tag, st, ms, surv in (("headline", host_stall, ms_per_step, stall_survives),
                                             ("secondary", (secondary or {}).get("host_stall_ms", 0.0),
                                              (secondary or {}).get("ms_per_step", 1.0),
                                              (secondary or {}).get("host_stall_survives_retries", False))) if surv]
            if bad:
                stall_check = "FAILED: the stall of the first attempt survived 3 timing attempts: " + "; ".join(bad)
        else:
            stall_check = "reported only (N > 1: rank skew and the exchange live in the same remainder; see per_rank)"
        # dominant kernel = the single-kernel stage with the largest time per step (a depth-sliced step
        # launches it once per slice: bytes and time are both summed over the step's launches)
        launches = {k: len(v) / n_stage_steps for k, v in stages.items()}
        single = {k: stage_ms[k] for k in ("raster_bwd", "raster_fwd", "project_fwd", "project_bwd") if k in stage_ms}
        dom = max(single, key=single.get)
        dom_source = "stage pass after the timed region"
        if dom == DOMINANT_STAGE and DOMINANT_STAGE in timed_dom:
            # the roofline uses the kernel's launches INSIDE the timed region
            single[dom] = round(sum(timed_dom[dom]) / args.steps, 4)
            launches[dom] = len(timed_dom[dom]) / args.steps
            dom_source = "HIP events around every launch of the kernel inside the timed region"
        P = S * R
        T = ((W + 15) // 16) * ((H + 15) // 16)
        # Algorithmic bytes.  Two bases are reported:
        #  * "emitted": the intersections actually placed in the launch's tile lists after depth slicing and
        #    exact tile culling — what the kernel can touch at all; this is the honest HBM-roofline basis;
        #  * "survey": SURVEY §8d's formula with the measured total I of the unsliced algorithm (every
        #    (Gaussian, tile) bounding-box pair) — the definition north_star's ">= 50 % of roofline" uses;
        #    the sliced path AVOIDS most of those bytes rather than streaming them.
        I_emit = int(sum(slice_isects)) if slice_isects else n_isect

        def alg_bytes(I):
            return {
                "raster_fwd": 40 * I + S * 20 * npix,
                "raster_bwd": 40 * I + S * 32 * npix + 36 * P * N,
                "project_fwd": 236 * N + 48 * P * N,
                "project_bwd": 84 * P * N + 2 * 236 * N,
            }

        def pipeline_bytes(I):
            a = alg_bytes(I)
            return (a["project_fwd"] + I * (12 + 24) + 8 * P * T + a["raster_fwd"] + 12 * npix + a["raster_bwd"] +
                    a["project_bwd"])

        alg, alg_survey = alg_bytes(I_emit), alg_bytes(n_isect)
        kname = {"raster_bwd": "raster_bwd_sload_kernel", "raster_fwd": "raster_fwd_sload_kernel",
                 "project_fwd": "project_fused_fwd_kernel", "project_bwd": "project_fused_bwd_sparse_kernel"}[dom]
        achieved = alg[dom] / (single[dom] * 1e-3) / 1e9
        traffic = None
        tfile = ROOT / "profiles" / "traffic.json"
        if tfile.exists():
            try:
                tj = json.loads(tfile.read_text())
                from gsdeblur_amd import _build as _gsd_build
                if tj.get("workload") == [N, W, H, S, R] and _counters_current(tj, _gsd_build, kname):
                    traffic = tj["hbm_bytes_per_step"].get(kname)
            except Exception:
                traffic = None
        # VALU issue side of the same kernel: wave-instructions per launch from the PMC pass
        # (profiles/traffic.json), priced (a) at the guide's 2 cycles per wave64 instruction and (b) at the issue rates
        # tools/valu_bench.hip measured for the kernel's own instruction mix (tools/valu_mix.py), over the 1024 SIMDs
        valu = None
        try:
            tj = json.loads(tfile.read_text()) if tfile.exists() else {}
            vi = tj.get("valu", {}).get(kname)
            from gsdeblur_amd import _build as _gsd_build
            fresh = _counters_current(tj, _gsd_build, kname)
            if vi and tj.get("workload") == [N, W, H, S, R] and not fresh:
                valu = {"stale": "profiles/traffic.json was measured on other kernel sources (kernel_source_hash differs): "
                                 "re-run tools/gpu_visit.sh <tag> pmc"}
            elif vi and tj.get("workload") == [N, W, H, S, R]:
                simd_cycles = single[dom] * 1e-3 * tj["valu"].get("clock_hz", 2.1e9) * 1024 / max(1.0, launches.get(dom, 1.0))
                valu = {"wave_instructions_per_launch": vi["insts_valu"],
                        "issue_frac_at_2_cycles": round(vi["insts_valu"] * 2.0 / simd_cycles, 4),
                        "mix_cycles_per_instruction": vi["mix_cycles_per_inst"],
                        "issue_frac_at_measured_mix": round(vi["insts_valu"] * vi["mix_cycles_per_inst"] / simd_cycles, 4),
                        # the same with the mix priced in wall ns (no clock assumed; the micro-benchmark's wall time
                        # includes its launch tails, so this one over-estimates: the truth lies between the two)
                        "issue_frac_at_measured_mix_wall_ns": (round(vi["insts_valu"] * vi["mix_wall_ns_per_inst"] /
                                                                     (simd_cycles / tj["valu"].get("clock_hz", 2.1e9) * 1e9), 4)
                                                               if "mix_wall_ns_per_inst" in vi else None),
                        "clock_hz_assumed": tj["valu"].get("clock_hz", 2.1e9),
                        "sq_wait_inst_any_frac": vi.get("wait_inst_any_frac"), "waves_per_simd": vi.get("waves_per_simd"),
                        "source": tj["valu"].get("source")}
        except Exception:
            valu = None
        counters_by = None
        try:
            if traffic is not None or (valu and "stale" not in valu):
                counters_by = ("kernel_source_hash (every kernel source as measured)" if tj.get("kernel_source_hash") ==
                               _gsd_build.kernel_source_hash() else
                               "kernel_isa_hash (this kernel's machine code as measured; other kernel sources changed since)")
        except Exception:
            counters_by = None
        roofline = {"bound": "hbm", "kernel": kname, "valu": valu, "counters_valid_by": counters_by,
                    "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": round(achieved / HBM_PEAK_GBS, 5), "traffic": traffic,
                    "algorithmic_basis": "intersections emitted into the tile lists (after depth slicing + exact "
                                         "tile culling); the kernel is VALU-issue-bound (roofline.valu), see DESIGN.md §5",
                    "algorithmic_bytes_per_step": alg[dom], "kernel_ms_per_step": single[dom],
                    "kernel_time_source": dom_source,
                    "launches_per_step": launches.get(dom, 1.0),
                    "avg_launch_ms": round(single[dom] / max(1.0, launches.get(dom, 1.0)), 4),
                    "pipeline_frac": round(pipeline_bytes(I_emit) / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 5),
                    "pipeline_algorithmic_bytes": pipeline_bytes(I_emit),
                    "survey_formula": {"note": "SURVEY §8d bytes with the total bounding-box intersection count I of "
                                               "the unsliced algorithm; most of these bytes are avoided, not streamed",
                                       "kernel_frac": round(alg_survey[dom] / (single[dom] * 1e-3) / 1e9 / HBM_PEAK_GBS, 5),
                                       "pipeline_bytes": pipeline_bytes(n_isect),
                                       "pipeline_frac": round(pipeline_bytes(n_isect) / (ms_per_step * 1e-3) / 1e9 /
                                                              HBM_PEAK_GBS, 5)}}
        lane_util = None
        lf = ROOT / "profiles" / "lane_stats.jsonl"
        if lf.exists():
            try:
                lane_util = {"source": "profiles/lane_stats.jsonl (tools/lane_stats.py: gs_rasterize_fwd_slice_stats "
                                       "counters of one forward per scene; committed measurement, not this run)"}
                for ln in lf.read_text().splitlines():
                    dj = json.loads(ln)
                    lane_util[dj["scene"]] = {k: dj[k] for k in ("pixel_utilisation_live", "blocks4x4_per_entry_geometric",
                                                                 "quads8x8_per_entry_geometric", "lockstep_speedup_4x4",
                                                                 "lockstep_speedup_8x8") if k in dj}
            except Exception:
                lane_util = None
        full_report = {
            "stage_ms": stage_ms,
            "host_stall_ms": round(host_stall, 4), "timing_attempts_ms": attempts,
            # first attempt, per step: ms until the host had issued it (the last entry is the closing synchronize)
            "host_issue_ms_per_step": first_issue_trace[:65] if host_stall > 0.10 * ms_per_step else None,
            "timing_attempt_reported": "first (retries only diagnose a host stall; they never replace the value)",
            "host_stall_check": stall_check,
            "stage_ms_source": f"{n_stage_steps} extra steps with HIP events around every stage, after the timed region",
            "roofline": roofline,
            "lane_utilisation": lane_util,
        }
        if world == 1 and not args.no_cpu_baseline:
            full_report["cpu_baseline"] = guarded_cpu_baseline()
    if rank == 0:
        line = {
            "metric": "fwd+bwd rasterize MPix/s at 1M Gaussians, 1080p, 5 sub-poses",
            "value": round(value, 3), "unit": "MPix/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"synthetic scene (SURVEY §8d, seed 1234): {N} Gaussians, {W}x{H}, "
                                   f"S={S} motion-blur sub-poses x R={R} row bands, SH degree 3, gamma 2.2, "
                                   f"fwd+bwd to all Gaussian params + viewmat + velocities"
                                   + ("" if args.view is None else f" — DIAGNOSTIC: camera {args.view % 16} of the view sweep, "
                                                                   f"not the headline view"),
                       "gaussians": N, "width": W, "height": H, "subposes": S, "rs_bands": R,
                       "motion_model": args.motion,
                       "tile_intersections_per_step": n_isect,
                       "tile_intersections_emitted": int(sum(slice_isects)) if ops.SLICE_BASE > 0 else n_isect,
                       "depth_slices": slice_isects if ops.SLICE_BASE > 0 else None,
                       "slice_budget": slice_budget,
                       "gaussians_with_gradient": rows_with_grad,
                       "api": ("ops.render_combined + Tensor.backward (torch.autograd; what model.get_outputs + "
                               "loss.backward() run)" if args.autograd else
                               "gsdeblur_amd.render_step: forward + backward of the frame in one host call — the entry "
                               "SplatfactoDeblurModel.render_and_backward / training.train_step call (same C-ABI calls as "
                               "the autograd node, no autograd engine between the compositors)"),
                       "frame_hints": headline_hints,
                       "views_per_step": world,
                       "parallelism": f"dp{world}" if world > 1 else "single",
                       "gradient_exchange": args.allreduce if (world > 1 or args.force_exchange) else None,
                       "gradient_exchange_forced_at_world_1": bool(args.force_exchange and world == 1),
                       "rccl_version": rccl_version, "per_rank": per_rank,
                       "subpose_MPix_per_s": round(value * S, 3),
                       "view_sweep": sweep,
                       "secondary": secondary},
            "exchange_ms": None if exchange_ms is None else round(exchange_ms, 4),
            "full": full,
        }
        if dumped is not None:
            line["outputs_dumped"] = {"dir": args.dump_outputs, "arrays": dumped}
        if full:
            line.update(full_report)
        print(json.dumps(line), flush=True)
    if world > 1 or args.force_exchange:
        dist.destroy_process_group()
    if rank == 0 and stall_check is not None and stall_check.startswith("FAILED"):
        # the line above carries the verdict (`host_stall_check`) and every attempt; the exit code only follows it on
        # request, so that a slow host still leaves a (flagged) measurement instead of none
        print(f"bench.py: {stall_check}", file=sys.stderr)
        if args.strict_stall:
            sys.exit(3)


if __name__ == "__main__":
    main()
