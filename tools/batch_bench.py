"""What rendering cameras in batches buys: bench.py's scene (1M Gaussians, 1920x1080, S = 5 blur samples) and its
16-camera view sweep (Workload.sweep_views(16)), rendered one camera per call (render_combined) and in batches of
B = 2, 4, 8, 16 (render_batch: one frame of B*S sub-poses).  For each batch size, after warm-up passes over the sweep:
forward-only ms per camera, forward + backward ms per camera (loss = sum over the cameras of a fixed weight . rgb), the
frame arena the batch leased and the peak device memory of the pass.  One JSON line per batch size.

    python tools/batch_bench.py [--passes 3] [--warmup 2] [--sizes 1,2,4,8,16]
    python tools/batch_bench.py --sizes 4 --passes 2 --mode fwdbwd     # one size and form (rocprofv3 --kernel-trace --stats)
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3, help="timed passes over the 16 cameras per form")
    ap.add_argument("--warmup", type=int, default=2, help="untimed passes before")
    ap.add_argument("--sizes", default="1,2,4,8,16")
    ap.add_argument("--mode", choices=("both", "fwd", "fwdbwd"), default="both")
    args = ap.parse_args()

    import torch
    import gsdeblur_amd as gs
    from gsdeblur_amd import ops
    import bench
    dev = torch.device("cuda:0")
    S, H, W, V = 5, 1080, 1920, 16
    wl = bench.Workload(gs, dev, 0, 1, 1_000_000, W, H, S, 1, "survey", "sparse")
    sc = wl.sc
    views = wl.sweep_views(V)
    times = torch.tensor(gs.subpose_schedule(S, 1 / 60, 1, 0.0)[0], device=dev)
    with torch.no_grad():
        vms_all = torch.stack([gs.subpose_viewmats(v[0], v[1], v[2], times) for v in views])     # [16, S, 4, 4]
    p = {k: v.detach().clone().requires_grad_(True) for k, v in wl.params.items()}
    wt = (torch.rand(V, H, W, 3, generator=torch.Generator().manual_seed(3)) - 0.5).to(dev) / (H * W)
    kw = dict(gamma=2.2, min_rgb_level=10.0)

    def render(B, k, grad):
        args_ = (p["means"], p["log_scales"].exp(), p["quats"], torch.sigmoid(p["opacity_logits"]), p["sh"])
        if B == 1:
            rgb = gs.render_combined(*args_, vms_all[k], None, S, 1, sc["fx"], sc["fy"], sc["cx"], sc["cy"], H, W,
                                     hints=hints[B].view(k), **kw)[0][None]
        else:
            rgb = gs.render_batch(*args_, vms_all[k:k + B], None, S, 1, sc["fx"], sc["fy"], sc["cx"], sc["cy"], H, W,
                                  hints=hints[B].view(k), **kw)[0]
        if grad:
            (wt[k:k + B] * rgb).sum().backward()

    def one_pass(B, grad):
        for k in range(0, V, B):
            if grad:
                for t in p.values():
                    t.grad = None
                render(B, k, True)
            else:
                with torch.no_grad():
                    render(B, k, False)

    def measure(B, res):
        for form in ("fwd", "fwdbwd"):
            if args.mode not in ("both", form):
                continue
            grad = form == "fwdbwd"
            for _ in range(args.warmup):
                one_pass(B, grad)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            ms = []
            for _ in range(args.passes):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                one_pass(B, grad)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3 / V)
            res[f"{form}_ms_per_camera"] = round(statistics.median(ms), 3)
            res[f"{form}_ms_per_camera_all"] = [round(v, 3) for v in ms]
            res[f"{form}_peak_mem_bytes"] = int(torch.cuda.max_memory_allocated(dev))


    sizes = [int(s) for s in args.sizes.split(",")]
    hints = {B: ops.FrameHints() for B in sizes}
    for B in sizes:
        res = {"batch": B, "cameras": V, "S": S, "gaussians": 1_000_000, "size": [W, H]}
        try:
            measure(B, res)
        except torch.OutOfMemoryError as e:
            # the frame arena grows with the batch's sub-pose count: a batch that does not fit is a result, not a crash
            res["error"] = "out of memory: " + str(e).split(".")[0]
            res["arena_bytes_wanted"] = int(hints[B].arena_bytes)
        else:
            res["arena_bytes"] = int(hints[B].arena_bytes)
        print(json.dumps(res), flush=True)
        for t in p.values():
            t.grad = None
        ops.release_arenas()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
