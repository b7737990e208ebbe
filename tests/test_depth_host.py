"""Host side of depth supervision (no GPU): the C ABI declares gs_frame_backward_depth and the ctypes table has it;
nerfstudio's depth fields in transforms.json, depth maps from .npy and 16-bit PNG, their undistortion / crop, the depth
downscale of the resolution schedule and the depth loss."""
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "3dgs-deblur_amd"


def test_header_declares_frame_backward_depth_and_ctypes_table_has_it(gs):
    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "gsdeblur.h").read_text(), flags=re.S)
    m = re.search(r"int\s+gs_frame_backward_depth\s*\(([^;]*)\)\s*;", txt)
    assert m, "gs_frame_backward_depth is not declared"
    args = [a for a in m.group(1).split(",") if a.strip()]
    base = re.search(r"int\s+gs_frame_backward\s*\(([^;]*)\)\s*;", txt)
    assert base and len(args) == len([a for a in base.group(1).split(",") if a.strip()]) + 1
    assert "v_depth" in args[-2] and "stream" in args[-1]
    lib = gs._lib
    assert "gs_frame_backward_depth" in lib._SIGS
    assert len(lib._SIGS["gs_frame_backward_depth"]) == len(args)
    assert lib._SIGS["gs_frame_backward_depth"][:-1] == lib._SIGS["gs_frame_backward"][:-1] + [lib._P]


def _write_scene(root: Path, frames_extra, top_extra=None):
    meta = {"w": 40, "h": 30, "fl_x": 50.0, "fl_y": 50.0, "cx": 20.0, "cy": 15.0, "frames": []}
    meta.update(top_extra or {})
    for i, extra in enumerate(frames_extra):
        fr = {"file_path": f"images/f{i:02d}.png", "transform_matrix": np.eye(4).tolist()}
        fr.update(extra)
        meta["frames"].append(fr)
    (root / "transforms.json").write_text(json.dumps(meta))


def test_load_transforms_reads_depth_fields(gs, tmp_path):
    _write_scene(tmp_path, [{"depth_file_path": "depth/f00.npy"}, {}, {"depth_file_path": "depth/f02.png"}],
                 {"depth_unit_scale_factor": 0.01})
    sc = gs.data.load_transforms(str(tmp_path))
    assert sc.depth_unit_scale_factor == pytest.approx(0.01)
    assert sc.depth_paths[0].endswith(str(Path("depth") / "f00.npy")) and sc.depth_paths[1] is None
    assert sc.depth_paths[2].endswith(str(Path("depth") / "f02.png"))
    _write_scene(tmp_path, [{}, {}])
    sc = gs.data.load_transforms(str(tmp_path))
    assert sc.depth_unit_scale_factor == pytest.approx(1e-3) and sc.depth_paths == [None, None]


def test_load_depth_npy_and_16bit_png(gs, tmp_path):
    from PIL import Image
    raw = np.random.default_rng(0).integers(0, 6000, size=(30, 40)).astype(np.uint16)
    raw[3, 4] = 0
    Image.fromarray(raw).save(tmp_path / "d.png")
    d = gs.data.load_depth(str(tmp_path / "d.png"), 1e-3)
    assert d.shape == (30, 40, 1) and d.dtype == torch.float32
    assert torch.allclose(d[..., 0], torch.from_numpy(raw.astype(np.float32)) * 1e-3)
    assert float(d[3, 4, 0]) == 0.0
    arr = raw.astype(np.float32)
    arr[0, 0], arr[0, 1] = np.nan, -5.0
    np.save(tmp_path / "d.npy", arr[..., None])
    e = gs.data.load_depth(str(tmp_path / "d.npy"), 2.0)
    assert e.shape == (30, 40, 1) and float(e[0, 0, 0]) == 0.0 and float(e[0, 1, 0]) == 0.0
    assert float(e[5, 5, 0]) == pytest.approx(2.0 * float(raw[5, 5]))


def test_scene_depths_follow_the_images_undistort_and_crop(gs, tmp_path):
    from PIL import Image
    _write_scene(tmp_path, [{"depth_file_path": "depth/f00.npy"}], {"k1": -0.2, "k2": 0.05})
    (tmp_path / "images").mkdir()
    (tmp_path / "depth").mkdir()
    Image.fromarray(np.full((30, 40, 3), 128, np.uint8)).save(tmp_path / "images" / "f00.png")
    dep = np.full((30, 40), 2000.0, np.float32)
    dep[:, :20] = 4000.0                 # two plateaus: nearest-neighbour sampling keeps exactly these two values
    dep[10:12, 30:32] = 0.0              # a hole stays a hole
    np.save(tmp_path / "depth" / "f00.npy", dep)
    sc = gs.data.load_transforms(str(tmp_path))
    cam0 = sc.cameras[0]
    d_before = gs.data.load_scene_depths(sc)[0]                  # cameras not yet replaced by the cropped ones
    imgs = gs.data.load_scene_images(sc)
    d_after = gs.data.load_scene_depths(sc)[0]                   # cameras now describe the cropped frame
    assert d_before.shape[:2] == imgs[0].shape[:2] == d_after.shape[:2]
    assert (sc.cameras[0].width, sc.cameras[0].height) == (d_after.shape[1], d_after.shape[0])
    assert torch.equal(d_before, d_after)
    vals = set(np.unique(d_after.numpy()).tolist())
    assert vals <= {0.0, 2.0, 4.0} and {2.0, 4.0} <= vals
    full = gs.data.undistort_depth(torch.from_numpy(dep)[..., None] * 1e-3, cam0.fx, cam0.fy, cam0.cx, cam0.cy,
                                   sc.distortion)
    assert full.shape == (30, 40, 1) and float((full == 0).float().sum()) > 0


def test_depth_downscale_keeps_invalid_pixels_out():
    T = _load_train_step()
    d = torch.zeros(4, 4, 1)
    d[0, 0, 0], d[0, 1, 0] = 2.0, 4.0            # block (0,0): two valid of four -> 3.0, not 1.5
    d[2:, 2:, 0] = 5.0                            # block (1,1): all valid
    out = T.downscale_depth(d, 2)
    assert out.shape == (2, 2, 1)
    assert out[0, 0, 0] == pytest.approx(3.0) and out[1, 1, 0] == pytest.approx(5.0)
    assert float(out[0, 1, 0]) == 0.0 and float(out[1, 0, 0]) == 0.0
    assert torch.equal(T.downscale_depth(d, 1), d)


def test_depth_loss_is_the_mean_over_valid_pixels():
    T = _load_train_step()
    gt = torch.tensor([[1.0, 0.0], [2.0, 3.0]])[..., None]
    pred = torch.tensor([[2.0, 9.0], [2.0, 1.0]])[..., None].requires_grad_(True)
    loss = T.depth_loss(pred, gt, 0.5)
    assert float(loss) == pytest.approx(0.5 * (1.0 + 0.0 + 2.0) / 3.0)
    loss.backward()
    assert float(pred.grad[0, 1, 0]) == 0.0 and float(pred.grad[0, 0, 0]) == pytest.approx(0.5 / 3.0)


def _load_train_step():
    import gsdeblur_amd
    return gsdeblur_amd.training
