"""What selective Adam saves: (1) the optimizer step alone at 1M Gaussians x 59 floats (widths 3, 3, 4, 1, 3, 45) —
dense gs_adam_step against gs_adam_step_rows at 0.5 %, 5 %, 33 % and 100 % selected rows, and the two mask builds
(gs_visible_rows over 5 radii planes, gs_dp_row_mask over the six gradients); (2) a whole train_step on bench.py's
headline scene (1M Gaussians, 1920x1080, S = 5) and on its fitted-model-like scene (profile "trained"), with
optimizer "adam" and "selective_adam" under both masks, and the rows each mask selects there.  The forms are
alternated in blocks within one process, so all see the same clocks; the line printed is JSON.

    python tools/selective_adam_bench.py [--steps 20] [--blocks 3] [--warmup 3] [--no-train]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

WIDTHS = [3, 3, 4, 1, 3, 45]


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


def optimizer_only(gs, dev, N: int, steps: int, blocks: int, warmup: int) -> dict:
    import torch
    L = gs._lib.load()
    g = torch.Generator(device=dev).manual_seed(0)
    ts = [[torch.randn(N, w, device=dev, generator=g) * s for s in (1.0, 0.1, 0.01, 0.001)] for w in WIDTHS]
    for t in ts:
        t[3].abs_()
    n = len(ts)
    vp = ctypes.c_void_p
    P = (vp * n)(*[t[0].data_ptr() for t in ts])
    G = (vp * n)(*[t[1].data_ptr() for t in ts])
    M = (vp * n)(*[t[2].data_ptr() for t in ts])
    V = (vp * n)(*[t[3].data_ptr() for t in ts])
    NE = (ctypes.c_longlong * n)(*[t[0].numel() for t in ts])
    W = (ctypes.c_int * n)(*WIDTHS)
    LR = (ctypes.c_float * n)(*([1e-9] * n))           # tiny steps: the parameters stay put over many repetitions
    ws_bytes = L.gs_adam_step_rows_workspace_bytes(N)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    stream = vp(torch.cuda.current_stream().cuda_stream)

    def dense():
        gs._lib.check(L.gs_adam_step(n, P, G, M, V, NE, LR, 0.9, 0.999, 1e-15, 10, stream), "adam_step")

    masks = []                          # keeps every mask alive while its closure runs

    def rows(mask):
        masks.append(mask)
        mp = vp(mask.data_ptr())
        return lambda: gs._lib.check(L.gs_adam_step_rows(n, N, mp, P, G, M, V, W, LR, 0.9, 0.999, 1e-15, 10,
                                                         vp(ws.data_ptr()), ws_bytes, stream), "adam_step_rows")
    forms = {"dense_gs_adam_step": dense}
    for share in (0.005, 0.05, 0.33, 1.0):
        mask = (torch.rand(N, device=dev, generator=g) < share).to(torch.uint8)
        forms[f"rows_{share * 100:g}pct"] = rows(mask)
    radii = torch.randint(-1, 3, (5, N), device=dev, generator=g, dtype=torch.int32)
    vis_mask = torch.empty(N, dtype=torch.uint8, device=dev)
    forms["mask_visible"] = lambda: gs._lib.check(L.gs_visible_rows(5, N, vp(radii.data_ptr()), vp(vis_mask.data_ptr()),
                                                                     stream), "visible_rows")
    grads = [t[1] for t in ts]
    ops = gs.dp._RowOps(grads)
    forms["mask_touched"] = ops.row_mask
    res = _alternate(forms, steps, blocks, warmup)
    return {"N": N, "floats_per_row": sum(WIDTHS), **{k: v["ms"] for k, v in res.items()},
            "blocks_ms": {k: v["blocks_ms"] for k, v in res.items()}}


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
    forms, models, rows = {}, {}, {}
    for tag, opt, kind in (("adam", "adam", "visible"), ("selective_visible", "selective_adam", "visible"),
                           ("selective_touched", "selective_adam", "touched")):
        cfg = gs.SplatfactoDeblurConfig(blur_samples=S, rolling_shutter_compensation=False, gamma=2.2,
                                        min_rgb_level=10.0, optimizer=opt, selective_mask=kind)
        model = gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev)
        opts = gs.training.make_optimizers(model)
        models[tag] = (model, opts)
        forms[tag] = (lambda m=model, o=opts: gs.training.train_step(m, o, cam, target, 0.2))
    res = _alternate(forms, steps, blocks, warmup)
    for tag in ("selective_visible", "selective_touched"):
        model, opts = models[tag]
        rows[tag.split("_")[1]] = int(gs.training.selection_mask(model, opts.values()).sum())
    return {"scene": profile, "N": N, "size": [W, H], "S": S, **{k + "_ms": v["ms"] for k, v in res.items()},
            "selected_rows": rows, "blocks_ms": {k: v["blocks_ms"] for k, v in res.items()}}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="timed repetitions per block")
    ap.add_argument("--blocks", type=int, default=3, help="blocks per form, alternated")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--no-train", action="store_true", help="the optimizer step alone")
    args = ap.parse_args()

    import torch
    import gsdeblur_amd as gs
    import bench
    dev = torch.device("cuda:0")
    out = {"optimizer_step": optimizer_only(gs, dev, args.gaussians, args.steps * 5, args.blocks, args.warmup)}
    torch.cuda.empty_cache()
    if not args.no_train:
        out["train_step"] = []
        for profile in ("survey", "trained"):
            out["train_step"].append(train_iteration(gs, bench, dev, profile, args.gaussians, 1920, 1080, 5, args.steps,
                                                     args.blocks, args.warmup))
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
