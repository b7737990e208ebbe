"""What the bilateral grid costs per training step on the MI355X: gs_bilagrid_slice_fwd + gs_bilagrid_slice_bwd and
gs_bilagrid_tv_fwd_bwd against the torch restatement of bilagrid.py on the same GPU tensors (forward + autograd backward:
the baseline the kernels replace), at 1080p and at the downscaled sizes of the resolution schedule, next to the
compulsory-traffic floor (60 B per pixel: rgb and v_out read, out and v_rgb written, rgb read again by the backward — at
the 8.0 TB/s peak), and a whole train_step with the grid on and off on bench.py's two scenes (1080p, S = 5; the grid-off
step is the step of the commit before the feature: it launches none of the new kernels).  The backward's cost depends on
how many (x cell, L cell) pairs a 64-pixel row segment holds, so the kernels are timed on a smooth picture (what a render
is) and on uniform noise (the worst case).  Forms are alternated in blocks within one process.  One JSON line, appended
to profiles/bilagrid_bench.jsonl with --record.

    python tools/bilagrid_step_bench.py [--steps 20] [--blocks 3] [--warmup 3] [--no-train] [--record]
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

PEAK_BYTES_PER_S = 8.0e12
BYTES_PER_PIXEL = 60
SIZES = ((1920, 1080), (960, 540), (480, 270))


def _timed(fn, n: int) -> float:
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / n


def _alternate(forms: dict, steps: int, blocks: int, warmup: int) -> dict:
    for f in forms.values():
        _timed(f, warmup)
    ms = {k: [] for k in forms}
    for _ in range(blocks):
        for k, f in forms.items():
            ms[k].append(_timed(f, steps))
    return {k: {"ms": round(statistics.median(v), 4), "blocks_ms": [round(x, 4) for x in v]} for k, v in ms.items()}


def _picture(kind: str, H: int, W: int, dev):
    import torch
    g = torch.Generator().manual_seed(11)
    if kind == "noise":
        return torch.rand(H, W, 3, generator=g).to(dev)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    img = torch.stack([0.15 + 0.7 * xx, 0.2 + 0.6 * yy, 0.5 + 0.3 * torch.sin(6 * xx + 3 * yy)], dim=-1)
    return (img + 0.01 * torch.randn(H, W, 3, generator=g)).clamp(0, 1).to(dev)


def kernels_only(dev, steps: int, blocks: int, warmup: int) -> list:
    import torch
    from gsdeblur_amd import bilagrid as BG
    rows = []
    g = torch.Generator().manual_seed(0)
    grids = (BG.identity_grids(4) + 0.05 * torch.randn(4, 12, 8, 16, 16, generator=g)).to(dev)
    idx = torch.tensor([2], dtype=torch.int32, device=dev)
    for W, H in SIZES:
        for kind in ("smooth", "noise"):
            rgb = _picture(kind, H, W, dev)[None].contiguous()
            v_out = torch.randn(1, H, W, 3, generator=g).to(dev)

            def hip():
                BG.slice_fwd_hip(grids, rgb, idx)
                BG.slice_bwd_hip(grids, rgb, idx, v_out)

            def hip_fwd():
                BG.slice_fwd_hip(grids, rgb, idx)

            def torch_form():
                gp, rp = grids.detach().requires_grad_(True), rgb.detach().requires_grad_(True)
                torch.autograd.grad(BG.slice_torch(gp, rp, idx), (rp, gp), v_out)
            res = _alternate({"slice_hip": hip, "slice_hip_fwd": hip_fwd, "slice_torch": torch_form}, steps, blocks, warmup)
            floor_ms = BYTES_PER_PIXEL * H * W / PEAK_BYTES_PER_S * 1e3
            rows.append({"size": [W, H], "picture": kind, **{k + "_ms": v["ms"] for k, v in res.items()},
                         "floor_ms_60B_per_pixel_at_8TBps": round(floor_ms, 4),
                         "slice_hip_over_floor": round(res["slice_hip"]["ms"] / floor_ms, 2),
                         "slice_torch_over_hip": round(res["slice_torch"]["ms"] / res["slice_hip"]["ms"], 2),
                         "blocks_ms": {k: v["blocks_ms"] for k, v in res.items()}})
    tv = []
    for G in (1, 100):
        gr = (BG.identity_grids(G) + 0.05 * torch.randn(G, 12, 8, 16, 16, generator=g)).to(dev)
        acc = torch.zeros_like(gr)

        def tv_torch_form():
            gp = gr.detach().requires_grad_(True)
            torch.autograd.grad(10.0 * BG.tv_torch(gp), gp)
        res = _alternate({"tv_hip": lambda: BG.tv_fwd_bwd_hip(gr, 10.0, acc), "tv_torch": tv_torch_form}, steps, blocks,
                         warmup)
        tv.append({"G": G, **{k + "_ms": v["ms"] for k, v in res.items()},
                   "tv_torch_over_hip": round(res["tv_torch"]["ms"] / res["tv_hip"]["ms"], 2),
                   "blocks_ms": {k: v["blocks_ms"] for k, v in res.items()}})
    return [{"slice": rows, "tv": tv}]


def train_iteration(gs, bench, dev, profile: str, N: int, W: int, H: int, S: int, steps: int, blocks: int,
                    warmup: int) -> dict:
    import torch
    sc = bench.make_scene(N, W, H, profile=profile)
    c2w = torch.eye(4)[:3].clone()
    c2w[:, 1] *= -1
    c2w[:, 2] *= -1
    cam = gs.Camera(c2w, sc["fx"], sc["fy"], sc["cx"], sc["cy"], W, H,
                    metadata=dict(cam_idx=0, camera_linear_velocity=[float(v) for v in sc["lin_vel"] * torch.tensor([1., -1., -1.])],
                                  camera_angular_velocity=[float(v) for v in sc["ang_vel"] * torch.tensor([1., -1., -1.])],
                                  exposure_time=sc["exposure_time"], rolling_shutter_time=0.0))
    target = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(7)).to(dev)
    forms = {}
    for tag, on in (("train_step", False), ("train_step_with_grid", True)):
        cfg = gs.SplatfactoDeblurConfig(blur_samples=S, rolling_shutter_compensation=False, gamma=2.2, min_rgb_level=10.0,
                                        use_bilateral_grid=on)
        model = gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev, num_cameras=100)
        opts = gs.training.make_optimizers(model, lr_scale=1e-3)      # the scene stays the scene that is timed
        forms[tag] = (lambda m=model, o=opts: gs.training.train_step(m, o, cam, target, 0.2))
    res = _alternate(forms, steps, blocks, warmup)
    return {"scene": profile, "N": N, "size": [W, H], "S": S, "grids": 100, **{k + "_ms": v["ms"] for k, v in res.items()},
            "grid_cost_ms": round(res["train_step_with_grid"]["ms"] - res["train_step"]["ms"], 4),
            "blocks_ms": {k: v["blocks_ms"] for k, v in res.items()}}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="timed repetitions per block")
    ap.add_argument("--blocks", type=int, default=3, help="blocks per form, alternated")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--no-train", action="store_true", help="the kernels alone")
    ap.add_argument("--record", action="store_true", help="append the result line to profiles/bilagrid_bench.jsonl")
    args = ap.parse_args()

    import torch
    import gsdeblur_amd as gs
    import bench
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "grid_shape": [16, 16, 8],
           "kernels": kernels_only(dev, args.steps, args.blocks, args.warmup)[0]}
    torch.cuda.empty_cache()
    if not args.no_train:
        out["train_step"] = []
        for profile in ("survey", "trained"):
            out["train_step"].append(train_iteration(gs, bench, dev, profile, args.gaussians, 1920, 1080, 5, args.steps,
                                                     args.blocks, args.warmup))
            torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.record:
        with open(ROOT / "profiles" / "bilagrid_bench.jsonl", "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
