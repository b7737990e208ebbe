"""What mesh decimation costs on the MI355X.

The meshes: the two of tools/mesh_clean_bench.py (the bench sphere with 300 floaters at 256^3 and 512^3, about 0.83 M and
2.82 M faces), extracted by gs.tsdf_extract_mesh.  Cases: cell_size = 2 and 4 voxels, and target_faces = 100000 with the
voxel size as the finest cell.  Alternated in blocks, medians of the blocks, after a warm-up of every form:

  call      gs.mesh_decimate end to end on the GPU mesh: the workspace, the plan(s) with their read-backs, the allocation of
            the outputs, emit
  plan      one gs_mesh_decimate_plan with the read-back of its counts, on a workspace that already exists
  emit      the allocation of the outputs and one gs_mesh_decimate_emit after that plan
  torch     gs.meshdecimate.mesh_decimate_torch on the same GPU tensors: the same rule as torch ops (torch.unique on the
            cell triples, index_add_ in float64, torch.linalg.solve, torch.unique on the sorted cluster triples)

Every time is a host clock around work that ends in a device synchronise.  Beside the times stand the integers of both
routes (they must agree), the largest position difference between them in float32 ulps, the workspace, and the compulsory
traffic: the bytes the op cannot avoid (verts, faces and colours read once; verts', colours', faces' and cluster_of written
once), with the time they take at the 6.3 TB/s a copy achieves on this GPU.  One JSON line, appended to
profiles/mesh_decimate_bench.jsonl with --record.

    python tools/mesh_decimate_bench.py [--steps 5] [--blocks 3] [--warmup 2] [--sizes 256 512] [--record]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

TARGET = 100000
ACHIEVABLE_BYTES_PER_S = 6.3e12


def compulsory_bytes(V, F, V_out, F_out):
    return 12 * V + 12 * F + 12 * V + 12 * V_out + 12 * V_out + 12 * F_out + 4 * V


def rows(gs, dev, n, args):
    import numpy as np
    import torch
    from mesh_clean_bench import _alternate, volume_with_floaters
    vol = volume_with_floaters(gs, dev, n)
    verts, faces, colors = gs.tsdf_extract_mesh(vol)
    vs = float(vol.voxel_size)
    V, F = int(verts.shape[0]), int(faces.shape[0])
    del vol
    torch.cuda.empty_cache()
    out = {"n": n, "V": V, "F": F, "voxel_size": vs, "cases": [],
           "workspace_MB": round(gs._lib.load().gs_mesh_decimate_workspace_bytes(V, F) / 1e6, 1)}
    cases = [("cell2", dict(cell_size=2 * vs)), ("cell4", dict(cell_size=4 * vs)), ("target", dict(cell_size=vs, target_faces=TARGET))]
    for name, kw in cases:
        got = gs.mesh_decimate(verts, faces, colors, return_map=True, return_stats=True, **kw)
        ref = gs.meshdecimate.mesh_decimate_torch(verts, faces, colors, return_map=True, return_stats=True, **kw)
        stats = got[4]
        scale = torch.maximum(ref[0].abs(), torch.full_like(ref[0], stats["cell_size"])).cpu().numpy()
        row = {"case": name, **stats,
               "integers_equal_torch": bool(torch.equal(got[1], ref[1]) and torch.equal(got[3], ref[3]) and got[4] == ref[4]),
               "position_ulps_vs_torch": round(float(((got[0] - ref[0]).abs().cpu().numpy() / np.spacing(scale)).max()), 2)
               if got[0].shape == ref[0].shape and len(got[0]) else None}
        run = gs.meshdecimate._Run(verts, faces, colors, True)
        used = stats["cell_size"]
        counts = run.plan(used)
        forms = {"call": lambda: gs.mesh_decimate(verts, faces, colors, **kw),
                 "plan": lambda: run.plan(used),
                 "emit": lambda: run.emit(counts),
                 "torch": lambda: gs.meshdecimate.mesh_decimate_torch(verts, faces, colors, **kw)}
        steps = {"call": args.steps, "plan": args.steps, "emit": args.steps, "torch": max(1, args.steps // 2)}
        res = _alternate(forms, steps, args.blocks, args.warmup)
        row.update({k + "_ms": v["ms"] for k, v in res.items()})
        row["blocks_ms"] = {k: v["blocks_ms"] for k, v in res.items()}
        row["torch_over_call"] = round(res["torch"]["ms"] / res["call"]["ms"], 2)
        b = compulsory_bytes(V, F, stats["verts_out"], stats["faces_out"])
        row["compulsory_MB"] = round(b / 1e6, 1)
        row["compulsory_ms_at_6.3TBps"] = round(b / ACHIEVABLE_BYTES_PER_S * 1e3, 4)
        out["cases"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del run, got, ref
        torch.cuda.empty_cache()
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5, help="timed calls per block")
    ap.add_argument("--blocks", type=int, default=3, help="blocks per form, alternated")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--record", action="store_true", help="append the result line to profiles/mesh_decimate_bench.jsonl")
    args = ap.parse_args()
    import torch
    import gsdeblur_amd as gs
    if not torch.cuda.is_available():
        raise SystemExit("mesh_decimate_bench.py measures on a GPU: none found")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "blocks": args.blocks, "warmup": args.warmup,
           "target_faces": TARGET, "meshes": []}
    for n in args.sizes:
        out["meshes"].append(rows(gs, dev, n, args))
    line = json.dumps(out)
    print(line)
    if args.record:
        with open(ROOT / "profiles" / "mesh_decimate_bench.jsonl", "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
