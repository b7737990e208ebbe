#!/usr/bin/env python
"""What persistence costs at benchmark size: wall time of checkpoint.save_checkpoint / load_checkpoint / export_ply and the
file sizes against their expected values, for N Gaussians at SH degree 3 with Adam state for all six groups (DESIGN.md
§5.8).  One JSON line per repetition.

  python tools/checkpoint_bench.py --gaussians 1000000 --reps 3 --dir /tmp/ckpt_bench
"""
import argparse
import json
import os
import sys
import tempfile
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import gsdeblur_amd as gs  # noqa: E402


def _timed(fn, dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default=os.path.join(tempfile.gettempdir(), "checkpoint_bench"),
                    help="where the two files are written (and removed again)")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    dev = torch.device(args.device)
    n = args.gaussians
    sc = gs.data.synthetic_scene(n, 1920, 1080, sh_degree=3, profile="trained")
    model = gs.SplatfactoDeblurModel.from_scene(gs.SplatfactoDeblurConfig(sh_degree=3), sc, dev)
    opts = gs.training.make_optimizers(model)
    for p in model.gauss_params().values():
        p.grad = torch.full_like(p, 1e-3)
    gs.training.optimizers_step(opts.values())                  # both moments exist for all six groups
    os.makedirs(args.dir, exist_ok=True)
    ck, ply = os.path.join(args.dir, "bench.pt"), os.path.join(args.dir, "bench.ply")
    floats = 3 + 3 + 4 + 1 + 3 + 45                             # 59 per Gaussian: 236 bytes
    for rep in range(args.reps):
        _, t_save = _timed(lambda: gs.checkpoint.save_checkpoint(ck, model, opts), dev)
        loaded, t_load = _timed(lambda: gs.checkpoint.load_checkpoint(ck, dev), dev)
        written, t_ply = _timed(lambda: gs.checkpoint.export_ply(ply, model), dev)
        assert loaded.model.num_points == n and written == n
        del loaded
        print(json.dumps({"gaussians": n, "device": str(dev), "rep": rep, "save_checkpoint_s": round(t_save, 3),
                          "load_checkpoint_s": round(t_load, 3), "export_ply_s": round(t_ply, 3),
                          "checkpoint_bytes": os.path.getsize(ck), "checkpoint_expected_tensor_bytes": 3 * 4 * floats * n,
                          "ply_bytes": os.path.getsize(ply),
                          "ply_expected_bytes": 248 * n + len(gs.checkpoint.ply_header(n, 45))}), flush=True)
    os.remove(ck)
    os.remove(ply)


if __name__ == "__main__":
    main()
