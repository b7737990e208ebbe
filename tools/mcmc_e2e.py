"""End-to-end check of 3DGS-MCMC densification at a fixed budget: the scene and seed cloud of tools/densify_e2e.py trained
without densification, with splatfacto's refinement schedule, and with MCMC whose cap_max is the size the splatfacto run
ended at — the like-for-like comparison an unbounded strategy cannot offer.  Sharp-frame PSNR / SSIM, the number of
Gaussians and the training seconds.  One scene, one seed.
usage: python tools/mcmc_e2e.py [iterations] [--record]   (--record appends the result to profiles/mcmc_train.jsonl)"""
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
from gsdeblur_amd import densify as D, mcmc as M   # noqa: E402

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
cap = None
for name in ("no_densification", "splatfacto", "mcmc"):
    reg = 0.0
    if name == "no_densification":
        dcfg = None
    elif name == "splatfacto":
        dcfg = D.DensifyConfig(warmup_length=200, refine_every=100, reset_alpha_every=8, stop_split_at=int(0.7 * iters),
                               stop_screen_size_at=int(0.3 * iters))
    else:
        dcfg = M.MCMCConfig(cap_max=cap, refine_start_iter=200, refine_every=100, refine_stop_iter=int(0.9 * iters))
        reg = 0.01
    cfg = gs.SplatfactoDeblurConfig(sh_degree=3, blur_samples=5, gamma=2.2, min_rgb_level=0.0,
                                    rolling_shutter_compensation=False, use_scale_regularization=True,
                                    opacity_reg=reg, scale_reg=reg)
    model = SD.init_from_seed_points(cfg, xyz, rgb, dev, num_cameras=len(scene.cameras))
    n0 = model.num_points
    r = gs.training.train_scene(model, scene, images, iters, densify=dcfg)
    if name == "splatfacto":
        cap = model.num_points
    res[name] = {"psnr": round(r["results"]["psnr"], 3), "ssim": round(r["results"]["ssim"], 4),
                 "gaussians": [n0, model.num_points], "seconds": round(r["wall_clock_time_seconds"], 2)}
    if name == "mcmc":
        res[name]["cap_max"] = cap
        res[name]["dead_share"] = round(float((torch.sigmoid(model.opacities.detach()) <= dcfg.min_opacity).float().mean()), 4)
    print(name, json.dumps(res[name]), flush=True)
line = json.dumps({"iterations": iters, "results": res})
print(line)
if record:
    with open(ROOT / "profiles" / "mcmc_train.jsonl", "a") as fh:
        fh.write(line + "\n")
