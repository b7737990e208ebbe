"""What TSDF fusion and mesh extraction cost on the MI355X.

Integration: 16 views of 1920 x 1080 (a ray-cast sphere in front of a backdrop, ring cameras) into a 256^3 and a 512^3
volume with colour: gs.tsdf_integrate in one call (one launch of kFramesPerLaunch = 16 frames), the same frames in 16
single-frame calls (what batching saves), and the baseline — gs.tsdf.tsdf_integrate_torch, the same rule as torch ops, on
the same GPU tensors — alternated in blocks.  Beside every time: the traffic floor (one read and one write of the 20-byte
voxel per launch at the measured 6.3 TB/s copy rate), the effective bytes per second of that traffic, and the ratios.
Extraction: the sphere's distance field at 256^3 and 512^3: gs_tsdf_mesh_count (count + scan) and gs_tsdf_mesh_emit
(vertices + faces) timed as calls.  The split into count, scan and emit kernels comes from a kernel trace of
`tools/tsdf_bench.py --extract-only` in a run of its own (rocprofv3 --kernel-trace --stats): the kernels are named
tsdf_count_kernel, tsdf_scan_{reduce,top,apply}_kernel, tsdf_verts_kernel and tsdf_faces_kernel.
The per-(block, frame) frustum reject was not built, so there is nothing to compare it with.
One JSON line, appended to profiles/tsdf_bench.jsonl with --record.

    python tools/tsdf_bench.py [--steps 3] [--blocks 3] [--warmup 1] [--sizes 256 512] [--extract-only] [--record]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import math
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

COPY_RATE = 6.3e12            # bytes / s, the measured device copy rate (MI355X_MICROARCH)
VOXEL_BYTES = 20              # tsdf, weight, three colour channels
VIEWS, H, W = 16, 1080, 1920


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


def frames(dev):
    """16 ring cameras around a sphere of radius 0.6 at the origin, a backdrop at depth 8 -> depth, colour, viewmats, intrins"""
    import torch
    views, intr = [], []
    for b in range(VIEWS):
        a = 0.1 + 2 * math.pi * b / VIEWS
        eye = torch.tensor([2.5 * math.cos(a), 2.5 * math.sin(a), 0.6])
        fwd = -eye / eye.norm()
        right = torch.linalg.cross(fwd, torch.tensor([0.0, 0.0, 1.0]))
        right = right / right.norm()
        down = torch.linalg.cross(fwd, right)
        R = torch.stack([right, down, fwd])
        m = torch.eye(4)
        m[:3, :3], m[:3, 3] = R, -R @ eye
        views.append(m)
        intr.append(torch.tensor([1400.0, 1400.0, W / 2, H / 2]))
    views, intr = torch.stack(views).to(dev), torch.stack(intr).to(dev)
    v, u = torch.meshgrid(torch.arange(H, device=dev) + 0.5, torch.arange(W, device=dev) + 0.5, indexing="ij")
    depth = torch.empty(VIEWS, H, W, device=dev)
    for b in range(VIEWS):
        d = torch.stack([(u - W / 2) / 1400.0, (v - H / 2) / 1400.0, torch.ones_like(u)], dim=-1)
        cc = views[b, :3, 3]                                  # the sphere's centre (the origin) in camera space
        a, bq = (d * d).sum(-1), d @ cc
        disc = bq * bq - a * (cc @ cc - 0.36)
        depth[b] = torch.where(disc > 0, (bq - disc.clamp(min=0).sqrt()) / a, torch.full_like(a, 8.0))
    color = torch.rand(VIEWS, H, W, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    return depth, color, views, intr


def integrate_rows(gs, dev, n, args):
    import torch
    depth, color, views, intr = frames(dev)
    vs = 2.0 / (n - 1)
    trunc = 4 * vs

    def fresh():
        return gs.TSDFVolume((-1.0, -1.0, -1.0), vs, (n, n, n), device=dev)
    vol = fresh()

    def batched():
        gs.tsdf_integrate(vol, depth, views, intr, trunc, color=color)

    def single():
        for b in range(VIEWS):
            gs.tsdf_integrate(vol, depth[b:b + 1], views[b:b + 1], intr[b:b + 1], trunc, color=color[b:b + 1])

    def baseline():
        gs.tsdf.tsdf_integrate_torch(vol, depth, views, intr, trunc, color=color)
    # the three forms give the same volume (the restatement up to the last bits of a float32 average)
    a, b, c = fresh(), fresh(), fresh()
    gs.tsdf_integrate(a, depth, views, intr, trunc, color=color)
    for f in range(VIEWS):
        gs.tsdf_integrate(b, depth[f:f + 1], views[f:f + 1], intr[f:f + 1], trunc, color=color[f:f + 1])
    gs.tsdf.tsdf_integrate_torch(c, depth, views, intr, trunc, color=color)
    row = {"n": n, "views": VIEWS, "image": [H, W], "touched_share": round(float((a.weight > 0).float().mean()), 4),
           "single_equals_batched": bool(torch.equal(a.tsdf, b.tsdf) and torch.equal(a.color, b.color)),
           "torch_max_abs_difference": float((a.tsdf - c.tsdf).abs().max()),
           "torch_weight_mismatch_share": float((a.weight != c.weight).float().mean())}
    del a, b, c
    torch.cuda.empty_cache()
    res = _alternate({"batched": batched, "single": single, "torch": baseline}, args.steps, args.blocks, args.warmup)
    traffic = 2.0 * VOXEL_BYTES * n ** 3
    for name, launches in (("batched", 1), ("single", VIEWS)):
        ms = res[name]["ms"]
        floor_ms = launches * traffic / COPY_RATE * 1e3
        row[name] = {"ms": ms, "blocks_ms": res[name]["blocks_ms"], "launches": launches, "floor_ms": round(floor_ms, 4),
                     "over_floor": round(ms / floor_ms, 2), "effective_TB_per_s": round(launches * traffic / (ms * 1e-3) / 1e12, 3)}
    row["torch"] = {"ms": res["torch"]["ms"], "blocks_ms": res["torch"]["blocks_ms"]}
    row["torch_over_batched"] = round(res["torch"]["ms"] / res["batched"]["ms"], 1)
    row["single_over_batched"] = round(res["single"]["ms"] / res["batched"]["ms"], 2)
    return row


def extract_rows(gs, dev, n, args):
    import torch
    from gsdeblur_amd import _lib
    lib = _lib.load()
    vs = 2.0 / (n - 1)
    ax = -1.0 + vs * torch.arange(n, device=dev)
    zz, yy, xx = torch.meshgrid(ax, ax, ax, indexing="ij")
    vol = gs.TSDFVolume((-1.0, -1.0, -1.0), vs, (n, n, n), device=dev)
    vol.tsdf.copy_((((xx - 0.03) ** 2 + (yy + 0.02) ** 2 + (zz - 0.04) ** 2).sqrt() - 0.6).div(4 * vs).clamp(-1, 1))
    vol.weight.fill_(1.0)
    vol.color.copy_(torch.stack([xx, yy, zz], dim=-1).mul(0.5).add(0.5))
    del xx, yy, zz
    verts, faces, _ = gs.tsdf_extract_mesh(vol)
    V, F = int(verts.shape[0]), int(faces.shape[0])
    vp = ctypes.c_void_p
    ws_bytes = int(lib.gs_tsdf_mesh_workspace_bytes(n, n, n))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    colors = torch.empty(V, 3, device=dev)
    stream = vp(torch.cuda.current_stream().cuda_stream)

    def count():
        _lib.check(lib.gs_tsdf_mesh_count(n, n, n, vp(vol.tsdf.data_ptr()), vp(vol.weight.data_ptr()), 0.0, 0.0,
                                          vp(counts.data_ptr()), vp(ws.data_ptr()), ws_bytes, stream), "count")

    def emit():
        _lib.check(lib.gs_tsdf_mesh_emit(n, n, n, -1.0, -1.0, -1.0, vs, vp(vol.tsdf.data_ptr()), vp(vol.color.data_ptr()), 0.0,
                                         V, F, vp(verts.data_ptr()), vp(faces.data_ptr()), vp(colors.data_ptr()),
                                         vp(ws.data_ptr()), ws_bytes, stream), "emit")
    res = _alternate({"count_call": count, "emit_call": emit, "extract": lambda: gs.tsdf_extract_mesh(vol)}, args.steps,
                     args.blocks, args.warmup)
    row = {"n": n, "V": V, "F": F, "workspace_MB": round(ws_bytes / 1e6, 1),
           "count_and_scan_ms": res["count_call"]["ms"], "emit_ms": res["emit_call"]["ms"],
           "extract_with_readback_and_allocation_ms": res["extract"]["ms"],
           "blocks_ms": {k: v["blocks_ms"] for k, v in res.items()}}
    return row


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3, help="timed calls per block")
    ap.add_argument("--blocks", type=int, default=3, help="blocks per form, alternated")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--record", action="store_true", help="append the result line to profiles/tsdf_bench.jsonl")
    ap.add_argument("--extract-only", action="store_true", help="skip the integration (for a kernel trace of the extraction)")
    args = ap.parse_args()

    import torch
    import gsdeblur_amd as gs
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "frames_per_launch": gs.tsdf.FRAMES_PER_LAUNCH, "integrate": [],
           "extract": []}
    for n in args.sizes:
        if not args.extract_only:
            out["integrate"].append(integrate_rows(gs, dev, n, args))
            print(json.dumps(out["integrate"][-1]), file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
        out["extract"].append(extract_rows(gs, dev, n, args))
        print(json.dumps(out["extract"][-1]), file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.record:
        with open(ROOT / "profiles" / "tsdf_bench.jsonl", "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
