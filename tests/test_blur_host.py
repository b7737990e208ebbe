"""Per-frame blur statistics and the blur-scored split on the CPU: csrc/blur_math.h compiled with g++ and blur_stats_torch
against the float64 reference (tests/blur_reference.py, whose docstring states the tolerance rule) on every case;
velocities_from_poses, the split rule and write_blur_scored against fixtures the REFERENCE made; the model and data
surface; the C-ABI entries."""
import ctypes
import inspect
import json
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import blur_reference as R

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "host_math" / "blur_host.cpp"
LIB = ROOT / "tests" / "host_math" / "libblur_host.so"
CSRC = ROOT / "3dgs-deblur_amd" / "csrc"
HDRS = [CSRC / "blur_math.h", CSRC / "gs_math.h"]
GOLDEN = ROOT / "tests" / "golden"
NEW_EXPORTS = {"gs_blur_stats_workspace_bytes": 2, "gs_blur_stats": 16, "gs_blur_stats_ppt": 17}
CASES = R.cases()
IDS = [c["name"] for c in CASES]


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def bh():
    if not LIB.exists() or LIB.stat().st_mtime < max(f.stat().st_mtime for f in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", f"-I{CSRC}", str(SRC),
                               "-o", str(LIB)])
    lib = ctypes.CDLL(str(LIB))
    lib.bh_default_clip.restype = ctypes.c_float
    lib.bh_blur_stats.restype = None
    lib.bh_blur_stats.argtypes = [ctypes.c_int] * 2 + [ctypes.c_void_p] * 6 + [ctypes.c_int] * 2 + [ctypes.c_float] + \
        [ctypes.c_void_p] * 2
    return lib


def as_dict(stats):
    return {"count": stats.count.cpu().numpy(), **{k: getattr(stats, k).cpu().numpy() for k in R.STATS}}


def tensors(c, device="cpu"):
    return [torch.from_numpy(c[k]).to(device) for k in ("points", "viewmats", "lin", "ang", "intrins", "times")]


def check_exact_zeros(c, got):
    """the `zeros` case: no exposure, no readout or no twist give exact zeros, not small numbers"""
    if c["name"] != "zeros":
        return
    assert (got["count"] > 0).all()
    for f, zero in ((0, ("mean_blur", "rms_blur", "max_blur")), (1, ("mean_skew",)), (2, R.STATS), (3, R.STATS)):
        for k in zero:
            assert got[k][f] == 0.0, (f, k, got[k][f])
    assert got["mean_skew"][0] > 0 and got["mean_blur"][1] > 0            # the T-only and the E-only frame


# --------------------------------------------------------------------------- #
# the statistic
# --------------------------------------------------------------------------- #
def test_the_cases_cover_what_they_claim():
    assert (R.CHUNK, R.FRAME_GROUP) == tuple(int(re.search(r"constexpr int %s = (\d+);" % k, HDRS[0].read_text()).group(1))
                                              for k in ("kChunk", "kFrameGroup"))
    by = {c["name"]: c for c in CASES}
    assert {by[f"N{n}"]["points"].shape[0] for n in (1, 63, 257, R.CHUNK - 1, R.CHUNK, R.CHUNK + 1, 3001)} == \
        {1, 63, 257, R.CHUNK - 1, R.CHUNK, R.CHUNK + 1, 3001}             # drop_fragile removed none of them
    assert [by[f"F{f}"]["viewmats"].shape[0] for f in (1, 31, 32, 33)] == [1, R.FRAME_GROUP - 1, R.FRAME_GROUP,
                                                                          R.FRAME_GROUP + 1]
    assert R.reference(by["looking_away"])["count"][3] == 0 and R.reference(by["looking_away"])["count"].max() > 2000
    assert R.reference(by["behind_camera_0"])["count"][0] == 0 and R.reference(by["behind_camera_0"])["count"].max() > 0
    assert len({tuple(r) for r in by["intrinsics"]["intrins"].tolist()}) == 7
    # the float32 evaluation's own error: below 1e-5 everywhere (a case above it would be ill-conditioned), and what the
    # reference module's docstring records
    measured = R.measured_errors()
    for k in R.STATS:
        assert 0 < measured[k] < 1e-5, (k, measured[k])
        assert measured[k] <= R.MEASURED[k] * 1.0001, (k, measured[k], "tests/blur_reference.py MEASURED is out of date")


def test_reference_is_first_order_in_the_exact_screw():
    c, scale = R.pin_case()
    exact, first, sel = R.exact_displacement(c, 2.0)
    assert (np.abs(exact - first) < 0.01 * first).all() and (first > 0.05).all(), (scale, exact, first)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_host_build_of_the_header(bh, c):
    F, N = c["viewmats"].shape[0], c["points"].shape[0]
    counts, stats = np.full(F, -1, np.int32), np.full((F, 4), -1, np.float32)
    bh.bh_blur_stats(F, N, P(c["points"]), P(c["viewmats"]), P(c["lin"]), P(c["ang"]), P(c["intrins"]), P(c["times"]),
                     c["W"], c["H"], c["clip"], P(counts), P(stats))
    got = {"count": counts, **{k: stats[:, i] for i, k in enumerate(R.STATS)}}
    R.check(c, got, "host")
    check_exact_zeros(c, got)
    assert abs(bh.bh_default_clip() - 0.01) < 1e-9 and bh.bh_chunk() == R.CHUNK and bh.bh_frame_group() == R.FRAME_GROUP


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_blur_stats_torch(gs, c):
    stats = gs.blur_stats(*tensors(c), c["W"], c["H"])                    # CPU tensors take blur_stats_torch
    assert stats.count.dtype == torch.int32 and all(getattr(stats, k).dtype == torch.float32 for k in R.STATS)
    got = as_dict(stats)
    R.check(c, got, "torch")
    check_exact_zeros(c, got)


def test_blur_stats_torch_chunks_over_frames(gs, monkeypatch):
    c = next(c for c in CASES if c["name"] == "F33")
    whole = gs.blur_stats(*tensors(c), c["W"], c["H"])
    monkeypatch.setattr(gs.blurscore, "_CHUNK_ELEMS", 5 * c["points"].shape[0])       # 5 frames at a time, then 3
    parts = gs.blur_stats(*tensors(c), c["W"], c["H"])
    for a, b in zip(whole, parts):
        assert torch.equal(a, b)


def test_blur_stats_argument_checks_and_empty_shapes(gs):
    c = CASES[1]
    t = tensors(c)
    with pytest.raises(ValueError, match=r"\[N,3\]"):
        gs.blur_stats(t[0][:, :2], *t[1:], 64, 48)
    with pytest.raises(ValueError, match="float32"):
        gs.blur_stats(t[0].double(), *t[1:], 64, 48)
    with pytest.raises(ValueError, match="times"):
        gs.blur_stats(*t[:5], t[5][:, :1], 64, 48)
    with pytest.raises(ValueError, match="no CPU fallback"):
        gs.blurscore.blur_stats_hip(*t, 64, 48)
    none = gs.blur_stats(t[0][:0], *t[1:], 64, 48)
    assert none.count.tolist() == [0] * 7 and all(float(getattr(none, k).abs().max()) == 0.0 for k in R.STATS)
    assert gs.blur_stats(t[0], *(x[:0] for x in t[1:]), 64, 48).count.shape == (0,)


# --------------------------------------------------------------------------- #
# velocities from poses
# --------------------------------------------------------------------------- #
def test_velocities_from_poses_against_the_reference_fixture(gs):
    d = json.load(open(GOLDEN / "ref_add_velocities.json"))
    assert len(d["cases"]) == 3 and {c["loop"] for c in d["cases"]} == {False, True}
    for case in d["cases"]:
        fr = case["frames"]
        c2w = torch.tensor([f["camera_to_world"] for f in fr], dtype=torch.float64)
        lin, ang = gs.data.velocities_from_poses(c2w, loop=case["loop"])
        assert lin.dtype == ang.dtype == torch.float64
        want_l = torch.tensor([f["camera_linear_velocity"] for f in fr], dtype=torch.float64)
        want_a = torch.tensor([f["camera_angular_velocity"] for f in fr], dtype=torch.float64)
        assert float((lin - want_l).abs().max()) < 1e-9 and float((ang - want_a).abs().max()) < 1e-9
        # times in seconds: the same path sampled at 30 Hz moves 30 times as fast
        n = len(fr)
        if not case["loop"]:
            l2, a2 = gs.data.velocities_from_poses(c2w[:, :3], times=[i / 30.0 for i in range(n)])
            assert torch.allclose(l2, 30.0 * want_l, rtol=1e-9, atol=1e-9)
            assert torch.allclose(a2, 30.0 * want_a, rtol=1e-9, atol=1e-9)
    lin, ang = gs.data.velocities_from_poses(torch.eye(4)[None])
    assert float(lin.abs().max()) == 0.0 and float(ang.abs().max()) == 0.0
    with pytest.raises(ValueError):
        gs.data.velocities_from_poses(torch.eye(4)[None].repeat(3, 1, 1), times=[0.0, 1.0, 0.0])


def test_so3_log_near_pi_and_zero(gs):
    from gsdeblur_amd.model import _so3_exp
    for w in ([0.0, 0.0, 0.0], [1e-9, 0.0, -2e-9], [0.3, -0.2, 0.9], [3.0, 0.5, -0.7],
              [np.pi - 1e-9, 0.0, 0.0], [0.0, -(np.pi - 1e-7), 0.0]):
        w = torch.tensor(w, dtype=torch.float64)
        got = gs.data._so3_log(_so3_exp(w)[None])[0]
        assert float((_so3_exp(got) - _so3_exp(w)).abs().max()) < 1e-9, (w, got)


# --------------------------------------------------------------------------- #
# the split
# --------------------------------------------------------------------------- #
def split_cases():
    return json.load(open(GOLDEN / "ref_blur_split.json"))["cases"]


def test_split_rule_and_write_blur_scored_against_the_reference_fixture(gs, tmp_path):
    cases = split_cases()
    assert [(len(c["input_transforms"]["frames"]), c["interval"]) for c in cases] == [(19, 8), (16, 4), (5, 8)]
    for ci, case in enumerate(cases):
        src, want = case["input_transforms"], case["output_transforms"]
        frames = sorted(src["frames"], key=lambda fr: fr["file_path"])
        if ci == 0:
            assert [fr["file_path"] for fr in src["frames"]] != [fr["file_path"] for fr in frames]     # out of order
            run = [fr["motion_blur_score"] for fr in frames[:8]]
            assert run.count(min(run)) == 2                                                            # a tie
        tr, ev = gs.data.split_indices([fr["file_path"] for fr in frames], "blur_score", case["interval"],
                                       [fr["motion_blur_score"] for fr in frames])
        want_ev = [i for i, fr in enumerate(want["frames"]) if os.path.basename(fr["file_path"]).startswith("eval_")]
        assert ev == want_ev and tr == [i for i in range(len(frames)) if i not in want_ev]
        # the written dataset: the JSON and the file list, and the files' bytes are the source images'
        root, dst = tmp_path / f"src{ci}", tmp_path / f"dst{ci}"
        os.makedirs(root / "images")
        for fr in src["frames"]:
            (root / fr["file_path"]).write_bytes(fr["file_path"].encode())
        (root / "sparse_pc.ply").write_text("ply\n")
        (root / "transforms.json").write_text(json.dumps(src))
        out = gs.data.write_blur_scored(str(root), str(dst), interval=case["interval"])
        assert json.load(open(out)) == want
        files = sorted(os.path.relpath(os.path.join(d, n), dst) for d, _, names in os.walk(dst) for n in names)
        assert files == case["files"]
        for fr_in, fr_out in zip(frames, want["frames"]):
            assert (dst / fr_out["file_path"]).read_bytes() == fr_in["file_path"].encode()
        # ... and reads back as the same split through the file names
        scene = gs.data.load_transforms(str(dst), eval_mode="filename")
        assert sorted(os.path.basename(scene.image_paths[i]) for i in scene.eval_indices) == \
            sorted(os.path.basename(f) for f in case["files"] if "eval_" in f)
        # scores handed over replace the stored ones: reversed scores choose other frames
        rev = [-fr["motion_blur_score"] for fr in frames]
        out2 = gs.data.write_blur_scored(str(root), str(tmp_path / f"rev{ci}"), scores=rev, interval=case["interval"])
        got2 = json.load(open(out2))
        assert [fr["motion_blur_score"] for fr in got2["frames"]] == rev
        assert [os.path.basename(fr["file_path"]).startswith("eval_") for fr in got2["frames"]] != \
            [os.path.basename(fr["file_path"]).startswith("eval_") for fr in want["frames"]]
    with pytest.raises(ValueError):
        gs.data.write_blur_scored(str(root), str(root))


def test_load_transforms_blur_score_mode(gs, tmp_path):
    case = split_cases()[0]
    src, want = case["input_transforms"], case["output_transforms"]
    (tmp_path / "transforms.json").write_text(json.dumps(src))
    scene = gs.data.load_transforms(str(tmp_path), eval_mode="blur_score", eval_interval=case["interval"])
    want_ev = [i for i, fr in enumerate(want["frames"]) if os.path.basename(fr["file_path"]).startswith("eval_")]
    assert scene.eval_indices == want_ev == [2, 9, 17]
    assert scene.train_indices == [i for i in range(19) if i not in want_ev]
    assert [c.metadata["is_eval"] for c in scene.cameras] == [i in want_ev for i in range(19)]
    broken = json.loads(json.dumps(src))
    del broken["frames"][4]["motion_blur_score"]
    (tmp_path / "transforms.json").write_text(json.dumps(broken))
    with pytest.raises(ValueError, match="motion_blur_score"):
        gs.data.load_transforms(str(tmp_path), eval_mode="blur_score")
    assert len(gs.data.load_transforms(str(tmp_path)).cameras) == 19          # the other modes do not need the score
    with pytest.raises(ValueError):
        gs.data.split_indices(["a", "b"], "blur_score", 8)
    with pytest.raises(ValueError):
        gs.data.split_indices(["a", "b"], "blur_score", 8, [1.0])


# --------------------------------------------------------------------------- #
# model and data surface
# --------------------------------------------------------------------------- #
def scene_of(gs, c):
    """the case as a dataset would hold it: OpenGL camera-to-world poses and velocities in metadata"""
    flip = np.array([1.0, -1.0, -1.0])
    cams = []
    for f in range(c["viewmats"].shape[0]):
        V = c["viewmats"][f].astype(np.float64)
        c2w = np.linalg.inv(V)
        c2w[:3, :3] = c2w[:3, :3] * flip[None, :]
        fx, fy, cx, cy = (float(v) for v in c["intrins"][f])
        md = dict(cam_idx=f, camera_linear_velocity=(c["lin"][f] * flip).tolist(),
                  camera_angular_velocity=(c["ang"][f] * flip).tolist(), exposure_time=float(c["times"][f, 0]),
                  rolling_shutter_time=float(c["times"][f, 1]))
        cams.append(gs.Camera(torch.tensor(c2w[:3], dtype=torch.float32), fx, fy, cx, cy, c["W"], c["H"], md))
    return gs.data.TransformsScene(cameras=cams, image_paths=[""] * len(cams), train_indices=[], eval_indices=[],
                                   exposure_time=R.E0, rolling_shutter_time=R.T0)


def model_of(gs, c, **cfg):
    n = c["points"].shape[0]
    config = gs.SplatfactoDeblurConfig(background_color="black", **cfg)
    return gs.SplatfactoDeblurModel(config, torch.from_numpy(c["points"]), torch.zeros(n, 3), torch.ones(n, 4), torch.zeros(n),
                                    torch.zeros(n, 3), torch.zeros(n, 15, 3), num_cameras=c["viewmats"].shape[0])


def test_data_blur_scores_and_model_blur_stats(gs):
    c = next(c for c in CASES if c["name"] == "intrinsics")
    scene = scene_of(gs, c)
    pts = torch.from_numpy(c["points"])
    scores = gs.data.blur_scores(scene, pts)
    ref = R.reference(c)
    # poses went through a float64 inverse and a float32 cast: the view matrices differ from the case's in the last bit
    assert isinstance(scores, list) and np.allclose(scores, ref["mean_blur"], rtol=2e-5, atol=0)
    stats = gs.data.blur_stats(scene, pts)
    assert np.abs(stats.count.numpy() - ref["count"]).max() <= 2
    # a model without adjustments: the same numbers, through the renderer's camera path
    # (its view matrix is a matrix-vector product where camera_arrays' is a batched one: the last bit may differ)
    model = model_of(gs, c)
    m = model.blur_stats(scene.cameras)
    assert int((m.count - stats.count).abs().max()) <= 2
    for k in R.STATS:
        assert torch.allclose(getattr(m, k), getattr(stats, k), rtol=2e-5, atol=0), k
    assert np.allclose(model.blur_scores(scene.cameras), scores, rtol=2e-5, atol=0)
    assert torch.equal(model.blur_stats(scene.cameras, points=pts[:100]).count, gs.data.blur_stats(scene, pts[:100]).count)
    # velocity adjustment: read by the statistic (frame 1 only)
    mv = model_of(gs, c, camera_velocity_optimizer=gs.model.CameraVelocityOptimizerConfig(enabled=True))
    s1 = mv.blur_scores(scene.cameras)
    assert np.allclose(s1, scores, rtol=2e-5, atol=0)
    with torch.no_grad():
        mv.velocity_adjustment[1] += torch.tensor([0.2, 0.0, 0.0, 0.0, 0.3, 0.0])
    s2 = mv.blur_scores(scene.cameras)
    assert abs(s2[1] - s1[1]) > 0.05 * s1[1] and s2[:1] + s2[2:] == s1[:1] + s1[2:]
    # zero_initial_velocities drops the data's velocities: what is left is the learned twist alone
    mz = model_of(gs, c, camera_velocity_optimizer=gs.model.CameraVelocityOptimizerConfig(enabled=True,
                                                                                          zero_initial_velocities=True))
    assert max(mz.blur_scores(scene.cameras)) == 0.0
    # exposure adjustment: E = E0 exp(adj) scales blur and leaves skew alone
    me = model_of(gs, c, camera_shutter_optimizer=gs.CameraShutterOptimizerConfig(exposure="global"))
    with torch.no_grad():
        me.exposure_adjustment[0] = float(np.log(2.0))
    e = me.blur_stats(scene.cameras)
    assert torch.allclose(e.mean_blur, 2.0 * stats.mean_blur, rtol=1e-5) and torch.allclose(e.mean_skew, stats.mean_skew,
                                                                                         rtol=1e-6)
    # a pose adjustment moves the camera: other points are visible
    mp = model_of(gs, c, camera_optimizer=gs.model.CameraOptimizerConfig(mode="SO3xR3"))
    with torch.no_grad():
        mp.pose_adjustment[2, 0] = 0.8
    assert int(mp.blur_stats(scene.cameras).count[2]) != int(stats.count[2])
    with pytest.raises(ValueError, match="one image size"):
        model.blur_stats([scene.cameras[0], scene.cameras[1].rescaled(2)])


def test_view_and_twist_is_the_models_conversion(gs):
    c = CASES[2]
    scene = scene_of(gs, c)
    model = model_of(gs, c)
    viewmats, lin, ang, intrins, times = gs.data.camera_arrays(scene.cameras)
    for f, cam in enumerate(scene.cameras):
        V, l, a = model._viewmat_and_velocity(cam)
        assert torch.allclose(V, viewmats[f], atol=1e-6) and torch.equal(l, lin[f]) and torch.equal(a, ang[f])
    assert torch.equal(intrins, torch.from_numpy(c["intrins"])) and torch.equal(times, torch.from_numpy(c["times"]))


def test_blur_score_tool_writes_scores_and_the_split(gs, tmp_path, capsys):
    import blur_score
    c = next(c for c in CASES if c["name"] == "N3001")
    scene = scene_of(gs, c)
    root = tmp_path / "scene"
    os.makedirs(root / "images")
    frames = []
    for f, cam in enumerate(scene.cameras):
        name = f"images/frame_{f:05d}.npy"
        np.save(root / name, np.zeros((2, 2, 3), np.float32))
        m = torch.cat([cam.camera_to_world, torch.tensor([[0.0, 0.0, 0.0, 1.0]])]).tolist()
        frames.append({"file_path": name, "transform_matrix": m,
                       "camera_linear_velocity": cam.metadata["camera_linear_velocity"],
                       "camera_angular_velocity": cam.metadata["camera_angular_velocity"]})
    gs.data.write_transforms(str(root), c["W"], c["H"], R.FOCAL, R.FOCAL, c["W"] / 2, c["H"] / 2, R.E0, R.T0, frames)
    pts = torch.from_numpy(c["points"])
    gs.data.write_seed_points_ply(str(root / "sparse_pc.ply"), pts, torch.full((len(pts), 3), 0.5), binary=True)
    want = gs.data.blur_scores(gs.load_transforms(str(root), eval_mode="all"), pts)
    assert np.allclose(want, R.reference(c)["mean_blur"], rtol=2e-5, atol=0)
    blur_score.main(["--data", str(root), "--device", "cpu", "--split-to", str(tmp_path / "split"), "--interval", "4"])
    split = gs.load_transforms(str(tmp_path / "split"), eval_mode="filename")
    assert [cam.metadata["motion_blur_score"] for cam in split.cameras if cam.metadata["is_eval"]] == \
        [min(want[:4]), min(want[4:])]
    assert (tmp_path / "split" / "sparse_pc.ply").exists() and len(split.train_indices) == 5
    blur_score.main(["--data", str(root), "--device", "cpu", "--write-scores"])
    scored = gs.load_transforms(str(root), eval_mode="blur_score", eval_interval=4)
    assert [cam.metadata["motion_blur_score"] for cam in scored.cameras] == want
    assert scored.eval_indices == [want.index(min(want[:4])), want.index(min(want[4:]))]
    # a trained model scores with what it learned: here a checkpoint of the seed cloud itself gives the same numbers
    ckpt = tmp_path / "model.ckpt"
    gs.checkpoint.save_checkpoint(str(ckpt), model_of(gs, c))
    capsys.readouterr()
    blur_score.main(["--data", str(root), "--device", "cpu", "--checkpoint", str(ckpt), "--split-to", str(tmp_path / "split2")])
    printed = [float(ln.split()[1]) for ln in capsys.readouterr().out.splitlines() if ln.startswith("frame_")]
    assert np.allclose(printed, want, rtol=1e-3)
    # pose-only data: finite differences of a static ring of cameras are not the stored twists
    blur_score.main(["--data", str(root), "--device", "cpu", "--from-poses", "--fps", "2", "--split-to", str(tmp_path / "split3")])
    printed = [float(ln.split()[1]) for ln in capsys.readouterr().out.splitlines() if ln.startswith("frame_")]
    assert len(printed) == 7 and min(printed) > 0 and not np.allclose(printed, want, rtol=1e-2)


# --------------------------------------------------------------------------- #
# exports
# --------------------------------------------------------------------------- #
def test_new_exports_and_their_argument_counts(gs):
    from gsdeblur_amd import _lib
    lib = _lib.load()
    sigs = {**_lib._SIGS, **_lib._SIGS_LL}
    for name, n in NEW_EXPORTS.items():
        assert hasattr(lib, name) and len(sigs[name]) == n, name
    assert lib.gs_blur_stats_workspace_bytes(7, 3001) == 3 * 7 * 32
    assert lib.gs_blur_stats_workspace_bytes(0, 5) == 0 and lib.gs_blur_stats_workspace_bytes(5, 0) == 0
    assert lib.gs_blur_stats_workspace_bytes(-1, 5) == -1 and lib.gs_blur_stats_workspace_bytes(5, -1) == -1
    assert lib.gs_blur_stats_workspace_bytes(65535 * 32 + 1, 5) == -1 and lib.gs_blur_stats_workspace_bytes(5, 2 ** 30 + 1) == -1
    # shapes beyond the grid limits and malformed arguments are refused before any launch (no GPU here: a launch would fail
    # with a hipError code >= 1000, not with 1)
    null = None
    assert lib.gs_blur_stats(65535 * 32 + 1, 5, null, null, null, null, null, null, 64, 48, 0.01, null, null, null, 0, null) == 1
    assert lib.gs_blur_stats(5, 5, null, null, null, null, null, null, 0, 48, 0.01, null, null, null, 0, null) == 1
    assert lib.gs_blur_stats(0, 5, null, null, null, null, null, null, 64, 48, 0.01, null, null, null, 0, null) == 0
    assert list(inspect.signature(gs.blur_stats).parameters) == ["points", "viewmats", "lin_vel", "ang_vel", "intrins", "times",
                                                                 "W", "H", "clip"]
    assert inspect.signature(gs.blur_stats).parameters["clip"].default == 0.01
    assert gs.blurscore.BlurStats._fields == ("count",) + R.STATS
    for fn, n in ((gs.data.blur_scores, 2), (gs.data.velocities_from_poses, 3), (gs.data.write_blur_scored, 4),
                  (gs.data.split_indices, 4), (gs.SplatfactoDeblurModel.blur_stats, 3),
                  (gs.SplatfactoDeblurModel.blur_scores, 2)):
        assert len(inspect.signature(fn).parameters) == n, fn
