"""End-to-end check of densification: the same seed-cloud start trained with and without the refinement
schedule on a blurred dataset; sharp-frame PSNR / SSIM and the number of Gaussians.  Rows: no densification, the signed
statistic, absgrad at the default threshold and absgrad at a four times higher one (same seed cloud, same iterations).
usage: python tools/densify_e2e.py [iterations] [--record]   (--record appends the result to profiles/absgrad_train.jsonl)"""
import json
import sys
import tempfile
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import gsdeblur_amd as gs          # noqa: E402
import synthetic_dataset as SD     # noqa: E402
from gsdeblur_amd import densify as D   # noqa: E402

record = "--record" in sys.argv
argv = [a for a in sys.argv[1:] if a != "--record"]
iters = int(argv[0]) if argv else 2000
dev = torch.device("cuda", 0)
root = tempfile.mkdtemp()
SD.generate(root, dev, width=240, height=160, n_frames=24, n_gaussians=8000, speed=1.0, dense_samples=32, seed_points=1500)
scene = gs.load_transforms(root)
images = gs.data.load_scene_images(scene, dev)
xyz, rgb = gs.load_seed_points_ply(scene.ply_file_path)
res = {}
sched = dict(warmup_length=200, refine_every=100, reset_alpha_every=8, stop_split_at=int(0.7 * iters),
             stop_screen_size_at=int(0.3 * iters))
thresh = D.DensifyConfig().densify_grad_thresh
for name, dcfg in (("no_densification", None),
                   ("densification", D.DensifyConfig(**sched)),
                   ("absgrad_default_thresh", D.DensifyConfig(absgrad=True, **sched)),
                   ("absgrad_4x_thresh", D.DensifyConfig(absgrad=True, densify_grad_thresh=4 * thresh, **sched))):
    cfg = gs.SplatfactoDeblurConfig(sh_degree=3, blur_samples=5, gamma=2.2, min_rgb_level=0.0,
                                    rolling_shutter_compensation=False, use_scale_regularization=True,
                                    densify_absgrad=bool(dcfg is not None and dcfg.absgrad))
    model = SD.init_from_seed_points(cfg, xyz, rgb, dev, num_cameras=len(scene.cameras))
    n0 = model.num_points
    r = gs.training.train_scene(model, scene, images, iters, densify=dcfg)
    res[name] = {"psnr": round(r["results"]["psnr"], 3), "ssim": round(r["results"]["ssim"], 4), "gaussians": [n0, model.num_points],
                 "seconds": round(r["wall_clock_time_seconds"], 2)}
    print(name, json.dumps(res[name]), flush=True)
line = json.dumps({"iterations": iters, "densify_grad_thresh": thresh, "results": res})
print(line)
if record:
    with open(ROOT / "profiles" / "absgrad_train.jsonl", "a") as fh:
        fh.write(line + "\n")
