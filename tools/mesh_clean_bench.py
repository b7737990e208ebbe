"""What mesh clean-up costs on the MI355X.

The mesh: the bench sphere of tools/tsdf_bench.py (radius 0.6 in a [-1, 1]^3 volume) with 300 small spheres of 1.5 to 3
voxels radius added to the field at seeded places outside it, at 256^3 and 512^3, extracted by gs.tsdf_extract_mesh.
Alternated in blocks, medians of the blocks:

  filter    gs.mesh_filter_components(keep_largest=1) end to end on the GPU mesh: the rounds with their read-backs, finish,
            plan, the read-back of the counts, the allocation of the outputs, emit
  labels    gs.mesh_components alone (rounds + finish + one read-back)
  extract   gs.tsdf_extract_mesh of the same volume (what produced the mesh)
  cpu       the same clean-up on the host, transfers included: faces to the host, connected components
            (scipy.sparse.csgraph.connected_components where scipy imports, else the numpy rounds of meshclean.py), the
            filter in numpy, the result back to the GPU; one call per block

The rounds taken and the component counts stand beside the times.  Per-kernel times come from a kernel trace in a run of
its own (`rocprofv3 --kernel-trace --stats -d DIR -- python tools/mesh_clean_bench.py --filter-only`; kernels mc_*_kernel
and the scan_*_kernel of the shared scan); `--kernel-stats FILE.csv` adds the rows of that trace's kernel statistics to the
record.  One JSON line, appended to profiles/mesh_clean_bench.jsonl with --record.

    python tools/mesh_clean_bench.py [--steps 5] [--blocks 3] [--warmup 2] [--sizes 256 512] [--filter-only] [--record]
"""
from __future__ import annotations

import argparse
import csv
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

FLOATERS = 300


def _timed(fn, n: int) -> float:
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / n


def _alternate(forms: dict, steps: dict, blocks: int, warmup: int) -> dict:
    for k, f in forms.items():
        _timed(f, min(warmup, steps[k]))
    ms = {k: [] for k in forms}
    for _ in range(blocks):
        for k, f in forms.items():
            ms[k].append(_timed(f, steps[k]))
    return {k: {"ms": round(statistics.median(v), 4), "blocks_ms": [round(x, 4) for x in v]} for k, v in ms.items()}


def volume_with_floaters(gs, dev, n):
    """the bench sphere of tools/tsdf_bench.py plus FLOATERS small spheres outside it -> TSDFVolume"""
    import torch
    vs = 2.0 / (n - 1)
    ax = -1.0 + vs * torch.arange(n, device=dev)
    zz, yy, xx = torch.meshgrid(ax, ax, ax, indexing="ij")
    vol = gs.TSDFVolume((-1.0, -1.0, -1.0), vs, (n, n, n), device=dev)
    vol.tsdf.copy_((((xx - 0.03) ** 2 + (yy + 0.02) ** 2 + (zz - 0.04) ** 2).sqrt() - 0.6).div(4 * vs).clamp(-1, 1))
    vol.weight.fill_(1.0)
    vol.color.copy_(torch.stack([xx, yy, zz], dim=-1).mul(0.5).add(0.5))
    del xx, yy, zz
    g = torch.Generator().manual_seed(11)
    placed = 0
    while placed < FLOATERS:
        c = torch.rand(3, generator=g) * 1.8 - 0.9
        r = float(1.5 + 1.5 * torch.rand(1, generator=g)) * vs
        if float((c - torch.tensor([0.03, -0.02, 0.04])).norm()) < 0.6 + 8 * vs + r:
            continue
        lo = [max(0, int((float(c[a]) - r + 1.0) / vs) - 5) for a in range(3)]
        hi = [min(n, int((float(c[a]) + r + 1.0) / vs) + 7) for a in range(3)]
        bz, by, bx = torch.meshgrid(ax[lo[2]:hi[2]], ax[lo[1]:hi[1]], ax[lo[0]:hi[0]], indexing="ij")
        d = (((bx - c[0]) ** 2 + (by - c[1]) ** 2 + (bz - c[2]) ** 2).sqrt() - r).div(4 * vs).clamp(-1, 1)
        box = vol.tsdf[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]
        box.copy_(torch.minimum(box, d))
        placed += 1
    return vol


def cpu_clean(gs, verts, faces, colors):
    """keep the largest component on the host, transfers included -> (the mesh on the GPU, the method's name)"""
    import numpy as np
    import torch
    dev = verts.device
    v, f, c = verts.cpu(), faces.cpu().numpy(), colors.cpu()
    V = len(v)
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        a = np.concatenate([f[:, 0], f[:, 1]])
        b = np.concatenate([f[:, 1], f[:, 2]])
        _, labels = connected_components(coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(V, V)), directed=False)
        method = "scipy.sparse.csgraph.connected_components"
    except ImportError:
        labels = gs.meshclean._rounds_numpy(f, V)[0]
        method = "numpy rounds"
    fcount = np.bincount(labels[f[:, 0]], minlength=int(labels.max()) + 1)
    keep_v = labels == int(fcount.argmax())
    keep_f = keep_v[f[:, 0]]
    new = (np.cumsum(keep_v) - 1).astype(np.int32)
    kv = torch.from_numpy(keep_v)
    out = (v[kv].to(dev), torch.from_numpy(new[f[keep_f]]).to(dev), c[kv].to(dev))
    return out, method


def rows(gs, dev, n, args):
    import torch
    vol = volume_with_floaters(gs, dev, n)
    verts, faces, colors = gs.tsdf_extract_mesh(vol)
    out = gs.mesh_filter_components(verts, faces, colors, keep_largest=1, return_stats=True)
    stats = out[3]
    row = {"n": n, "V": int(verts.shape[0]), "F": int(faces.shape[0]), "floaters": FLOATERS, **stats,
           "workspace_MB": round(gs._lib.load().gs_mesh_clean_workspace_bytes(len(verts), len(faces)) / 1e6, 1)}
    forms = {"filter": lambda: gs.mesh_filter_components(verts, faces, colors, keep_largest=1)}
    steps = {"filter": args.steps}
    if not args.filter_only:
        (cv, cf, cc), method = cpu_clean(gs, verts, faces, colors)
        row["cpu_method"] = method
        row["cpu_equals_gpu"] = bool(torch.equal(cv, out[0]) and torch.equal(cf, out[1]) and torch.equal(cc, out[2]))
        forms.update({"labels": lambda: gs.mesh_components(faces, len(verts)),
                      "extract": lambda: gs.tsdf_extract_mesh(vol),
                      "cpu": lambda: cpu_clean(gs, verts, faces, colors)})
        steps.update({"labels": args.steps, "extract": args.steps, "cpu": 1})
    res = _alternate(forms, steps, args.blocks, args.warmup)
    row.update({k + "_ms": v["ms"] for k, v in res.items()})
    row["blocks_ms"] = {k: v["blocks_ms"] for k, v in res.items()}
    if not args.filter_only:
        row["filter_over_extract"] = round(res["filter"]["ms"] / res["extract"]["ms"], 2)
        row["cpu_over_filter"] = round(res["cpu"]["ms"] / res["filter"]["ms"], 1)
    return row


def kernel_stats(path):
    """the rows of a rocprofv3 kernel-statistics CSV that belong to the clean-up (mc_* and the shared scan)"""
    with open(path, newline="") as fh:
        return [r for r in csv.DictReader(fh) if any("mc_" in str(v) or "scan_" in str(v) for v in r.values())]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5, help="timed calls per block")
    ap.add_argument("--blocks", type=int, default=3, help="blocks per form, alternated")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--filter-only", action="store_true", help="only the GPU clean-up (for a kernel trace)")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 kernel-statistics CSV of a --filter-only run to record")
    ap.add_argument("--record", action="store_true", help="append the result line to profiles/mesh_clean_bench.jsonl")
    args = ap.parse_args()

    if args.kernel_stats:
        out = {"kernel_trace": kernel_stats(args.kernel_stats), "sizes": args.sizes, "steps": args.steps, "blocks": args.blocks,
               "warmup": args.warmup}
    else:
        import torch
        import gsdeblur_amd as gs
        dev = torch.device("cuda:0")
        out = {"device": torch.cuda.get_device_name(0), "filter_only": args.filter_only, "meshes": []}
        for n in args.sizes:
            out["meshes"].append(rows(gs, dev, n, args))
            print(json.dumps(out["meshes"][-1]), file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.record:
        with open(ROOT / "profiles" / "mesh_clean_bench.jsonl", "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
