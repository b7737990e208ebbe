"""Persistence: training checkpoints (save / resume) and the Gaussian-splat PLY that viewers read.

The reference delegates both to nerfstudio ("model state = Gaussian params"; three of its entry points
start from ``--load-config``: its train.py:87-95, render_model.py:171, render_video.py:261-276).  This
project has its own trainer, so it has its own files.  Host code only: no kernel, nothing on the training hot path.

Checkpoint (``save_checkpoint`` / ``load_checkpoint``): ONE ``torch.save`` of a plain dict — tensors (on the CPU), ints,
floats, bools, strings, lists, dicts and None, nothing else — so that ``torch.load(..., weights_only=True)`` reads it; there
is no fallback to full unpickling.  Layout (version 1):

    format "gsdeblur-checkpoint", version 1
    model       config (dataclasses.asdict of SplatfactoDeblurConfig), num_cameras, step, params {the six gauss_params},
                background_param / pose_adjustment / velocity_adjustment / bilateral_grids (tensor or None);
                exposure_adjustment / readout_adjustment (tensor) ONLY when the shutter optimizer has them
    optimizers  None, or {"kind": "adam" | "selective_adam", "groups": {name: lr, betas, eps, step, exp_avg, exp_avg_sq}}
    trainer     None, or train_scene's loop state (trainer_state)
    densify_state  None, or DensifyState's accumulators
    extra       None, or whatever plain data the caller adds

The model is REBUILT at the saved row count: densification and MCMC change N, so a checkpoint cannot be a
``load_state_dict`` into a model of the initial size.  Transient attributes are not saved: ``radii``, ``xy_grad``,
``xy_absgrad`` belong to the last render, and ``frame_hints`` (ops.FrameHints) is performance memory — slice budgets and
arena estimates that a few frames relearn; a loaded model starts with a fresh one and renders the same values.

The optimizer state layout is shared by torch.optim.Adam, train_step.SelectiveAdam and fused.HipAdam (state keys
``step`` / ``exp_avg`` / ``exp_avg_sq``); only the step count differs — HipAdam keeps an int, the two torch forms a float
tensor.  The file holds an int and the loader restores whichever form the class wants, so a checkpoint written from GPU
optimizers loads into CPU ones and the other way round.

Gaussian-splat PLY (``export_ply`` / ``load_ply``): the layout of the original 3DGS code and of nerfstudio's
``ns-export gaussian-splat``.  No exporter exists in the reference tree; the property list below is a RECOLLECTION, like
SURVEY App. A.
"""
from __future__ import annotations

import dataclasses
import os
import re
import tempfile
from typing import Any, Dict, List, Optional

import torch
from torch import Tensor

from .model import (CameraOptimizerConfig, CameraShutterOptimizerConfig, CameraVelocityOptimizerConfig,
                    SplatfactoDeblurConfig, SplatfactoDeblurModel)

FORMAT = "gsdeblur-checkpoint"
VERSION = 1

GAUSS_NAMES = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")
SMALL_NAMES = ("background_param", "pose_adjustment", "velocity_adjustment", "bilateral_grids")
# the shutter optimizer's parameters: their keys are written ONLY when the parameter exists (a file of a model without
# them has exactly the keys it always had), and a file without the keys loads as "off"
SHUTTER_NAMES = ("exposure_adjustment", "readout_adjustment")


# --------------------------------------------------------------------------- #
# plain data
# --------------------------------------------------------------------------- #
def _plain(obj: Any, where: str = "checkpoint") -> Any:
    """obj as the file may hold it: tensors detached on the CPU, tuples as lists; anything outside the allowed set is a
    TypeError naming where it sits (weights_only loading would refuse the file later, far from the cause)"""
    if obj is None or isinstance(obj, (bool, int, float, str)):
        return obj
    if isinstance(obj, Tensor):
        return obj.detach().to("cpu").contiguous().clone()
    if isinstance(obj, (list, tuple)):
        return [_plain(v, f"{where}[{i}]") for i, v in enumerate(obj)]
    if isinstance(obj, dict):
        for k in obj:
            if not isinstance(k, (str, int)):
                raise TypeError(f"{where}: dict key {k!r} is neither a string nor an int")
        return {k: _plain(v, f"{where}.{k}") for k, v in obj.items()}
    raise TypeError(f"{where}: a checkpoint holds tensors, ints, floats, bools, strings, lists, dicts and None, "
                    f"not {type(obj).__name__}")


def _serialize(obj: Dict, f) -> None:
    torch.save(obj, f)


def _atomic_write(path: str, write) -> None:
    """write(file) into a temporary file beside `path`, then os.replace: a failure half way leaves the previous file
    as it was and no temporary file behind"""
    path = os.fspath(path)
    folder = os.path.dirname(os.path.abspath(path))
    os.makedirs(folder, exist_ok=True)
    fd, tmp = tempfile.mkstemp(dir=folder, prefix=os.path.basename(path) + ".", suffix=".tmp")
    try:
        with os.fdopen(fd, "wb") as f:
            write(f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise


# --------------------------------------------------------------------------- #
# config
# --------------------------------------------------------------------------- #
def config_to_dict(config: SplatfactoDeblurConfig) -> Dict:
    """dataclasses.asdict with the nested optimizer configs as dicts and grid_shape as a list"""
    d = dataclasses.asdict(config)
    d["grid_shape"] = [int(v) for v in d["grid_shape"]]
    return d


_NESTED = {"camera_optimizer": CameraOptimizerConfig, "camera_velocity_optimizer": CameraVelocityOptimizerConfig,
           "camera_shutter_optimizer": CameraShutterOptimizerConfig}


def _dataclass_from_dict(cls, d: Dict, where: str):
    names = {f.name for f in dataclasses.fields(cls)}
    for k in d:
        if k not in names:
            raise ValueError(f"{where}: unknown key {k!r} (written by a newer version?)")
    return cls(**d)


def config_from_dict(d: Dict) -> SplatfactoDeblurConfig:
    """a missing key takes the dataclass default (old files survive new fields); an unknown key is a ValueError"""
    d = dict(d)
    for k, cls in _NESTED.items():
        if k in d:
            d[k] = _dataclass_from_dict(cls, dict(d[k]), f"config.{k}")
    if "grid_shape" in d:
        d["grid_shape"] = tuple(int(v) for v in d["grid_shape"])
    return _dataclass_from_dict(SplatfactoDeblurConfig, d, "config")


# --------------------------------------------------------------------------- #
# sections
# --------------------------------------------------------------------------- #
def _model_section(model: SplatfactoDeblurModel) -> Dict:
    sec = {"config": config_to_dict(model.config), "num_cameras": int(model.num_cameras), "step": int(model.step),
           "params": {k: p.data for k, p in model.gauss_params().items()}}
    for k in SMALL_NAMES:
        p = getattr(model, k, None)
        sec[k] = None if p is None else p.data
    for k in SHUTTER_NAMES:
        p = getattr(model, k, None)
        if p is not None:
            sec[k] = p.data
    return sec


def optimizer_kind(optimizers: Dict[str, torch.optim.Optimizer]) -> str:
    """make_optimizers' `optimizer` argument that built these: "selective_adam" iff the Gaussian groups are selective"""
    o = optimizers.get("means")
    return "selective_adam" if o is not None and getattr(o, "selective", False) else "adam"


def _optimizers_section(optimizers: Dict[str, torch.optim.Optimizer]) -> Dict:
    groups = {}
    for name, opt in optimizers.items():
        if len(opt.param_groups) != 1 or len(opt.param_groups[0]["params"]) < 1:
            raise ValueError(f"optimizer {name!r}: one parameter group expected (make_optimizers' layout)")
        grp = opt.param_groups[0]
        rec = {"lr": float(grp["lr"]), "betas": [float(b) for b in grp["betas"]], "eps": float(grp["eps"])}
        states = []
        for param in grp["params"]:
            st = opt.state.get(param, None)
            one = {"step": None, "exp_avg": None, "exp_avg_sq": None}
            if st:
                # HipAdam: int; torch.optim.Adam / SelectiveAdam: float tensor — the file holds an int
                one["step"] = int(st["step"])
                one["exp_avg"], one["exp_avg_sq"] = st["exp_avg"], st["exp_avg_sq"]
            states.append(one)
        if len(states) == 1:
            rec.update(states[0])
        else:
            # a group of several parameters ("camera_shutter_opt"): the three state keys hold lists, in parameter order
            for key in ("step", "exp_avg", "exp_avg_sq"):
                rec[key] = [one[key] for one in states]
        groups[name] = rec
    return {"kind": optimizer_kind(optimizers), "groups": groups}


def _densify_section(state) -> Dict:
    return {"xys_grad_norm": state.xys_grad_norm, "vis_counts": state.vis_counts, "max_2Dsize": state.max_2Dsize,
            "size": [int(state.size[0]), int(state.size[1])], "absgrad": bool(state.absgrad)}


def trainer_state(iteration: int, seed: int, generator: Optional[torch.Generator], order, ev_pos: int, history,
                  wall_clock_time_seconds: float, lr_scale: float, ssim_lambda: float, densify=None,
                  device=None) -> Dict:
    """train_scene's loop state as a checkpoint's `trainer` section: the iteration reached, the shuffle generator's state
    and what is left of the current pass (`order`), the evaluation-camera cursor, the log, the time spent so far, which
    densification strategy ran (None / "splatfacto" / "mcmc") with its config, and the DEFAULT generators' states — the
    CPU one, and the CUDA one of `device` when that is a GPU (background_color="random" draws from it).
    MCMC keeps no state of its own: every draw is keyed by (seed, step)."""
    from . import mcmc as M
    strategy, strategy_config = None, None
    if densify is not None:
        strategy = "mcmc" if isinstance(densify, M.MCMCConfig) else "splatfacto"
        strategy_config = dataclasses.asdict(densify)
    dev = torch.device(device) if device is not None else None
    return {"iteration": int(iteration), "seed": int(seed),
            "generator_state": None if generator is None else generator.get_state(),
            "order": [int(i) for i in order], "ev_pos": int(ev_pos), "history": _plain(list(history), "history"),
            "wall_clock_time_seconds": float(wall_clock_time_seconds), "lr_scale": float(lr_scale),
            "ssim_lambda": float(ssim_lambda), "strategy": strategy, "strategy_config": strategy_config,
            "rng_cpu": torch.get_rng_state(),
            "rng_cuda": torch.cuda.get_rng_state(dev) if dev is not None and dev.type == "cuda" else None}


def restore_default_generators(trainer: Dict, device=None) -> None:
    """set the default CPU generator, and `device`'s default CUDA generator when the file holds one and `device` is a
    GPU, to the saved states"""
    if trainer.get("rng_cpu") is not None:
        torch.set_rng_state(trainer["rng_cpu"].to(torch.uint8).cpu())
    dev = torch.device(device) if device is not None else None
    if trainer.get("rng_cuda") is not None and dev is not None and dev.type == "cuda":
        torch.cuda.set_rng_state(trainer["rng_cuda"].to(torch.uint8).cpu(), dev)


def save_checkpoint(path, model: SplatfactoDeblurModel, optimizers: Optional[Dict[str, torch.optim.Optimizer]] = None,
                    trainer: Optional[Dict] = None, densify_state=None, extra: Optional[Dict] = None) -> None:
    """Write one checkpoint file (module docstring: layout).  optimizers: make_optimizers' dict; trainer: a plain dict,
    train_scene passes trainer_state(...); densify_state: a densify.DensifyState; extra: plain data of the caller's.
    The write is atomic (temporary file in the same directory, then os.replace).  Not saved: radii, xy_grad, xy_absgrad
    and frame_hints — the last is performance memory that a few frames relearn."""
    obj = {"format": FORMAT, "version": VERSION,
           "model": _model_section(model),
           "optimizers": None if optimizers is None else _optimizers_section(optimizers),
           "trainer": trainer,
           "densify_state": None if densify_state is None else _densify_section(densify_state),
           "extra": extra}
    obj = _plain(obj)
    _atomic_write(path, lambda f: _serialize(obj, f))


class Checkpoint:
    """what load_checkpoint returns: .model, .optimizers (dict or None), .trainer (dict or None), .densify_state
    (densify.DensifyState or None), .extra"""

    def __init__(self, model, optimizers, trainer, densify_state, extra):
        self.model, self.optimizers, self.trainer = model, optimizers, trainer
        self.densify_state, self.extra = densify_state, extra


def _check_header(obj) -> None:
    if not isinstance(obj, dict) or obj.get("format") != FORMAT:
        got = obj.get("format") if isinstance(obj, dict) else type(obj).__name__
        raise ValueError(f"not a {FORMAT} file (format {got!r})")
    version = obj.get("version")
    if not isinstance(version, int) or version < 1 or version > VERSION:
        raise ValueError(f"checkpoint version {version!r}: this code reads versions 1..{VERSION}")


def _build_model(sec: Dict, device) -> SplatfactoDeblurModel:
    config = config_from_dict(sec["config"])
    p = sec["params"]
    missing = [k for k in GAUSS_NAMES if k not in p]
    if missing:
        raise ValueError(f"checkpoint misses the Gaussian parameters {missing}")
    model = SplatfactoDeblurModel(config, p["means"], p["scales"], p["quats"], p["opacities"], p["features_dc"],
                                  p["features_rest"], num_cameras=int(sec["num_cameras"]))
    _fill_small(model, sec)
    model.step = int(sec["step"])
    return model.to(device)


def _fill_small(model: SplatfactoDeblurModel, sec: Dict) -> None:
    with torch.no_grad():
        for k in SMALL_NAMES + SHUTTER_NAMES:
            saved, have = sec.get(k), getattr(model, k, None)
            if (saved is None) != (have is None):
                raise ValueError(f"checkpoint and config disagree about {k}: "
                                 f"{'absent' if saved is None else 'present'} in the file")
            if saved is not None:
                if tuple(saved.shape) != tuple(have.shape):
                    raise ValueError(f"{k}: shape {tuple(saved.shape)} in the file, {tuple(have.shape)} in the model")
                have.copy_(saved.to(have.device))


def _restore_into(model: SplatfactoDeblurModel, sec: Dict) -> None:
    """the saved state into an existing model of the same config: the six Gaussian parameters are REPLACED by
    parameters of the saved row count, the small ones copied"""
    saved_cfg, own_cfg = config_to_dict(config_from_dict(sec["config"])), config_to_dict(model.config)
    # color_corrected_metrics only chooses what evaluate() reports: a run may be resumed with it switched either way
    diff = sorted(k for k in saved_cfg if saved_cfg[k] != own_cfg.get(k) and k != "color_corrected_metrics")
    if diff:
        raise ValueError(f"the checkpoint's config differs from the model's in {diff}")
    if int(sec["num_cameras"]) != int(model.num_cameras):
        raise ValueError(f"checkpoint of {int(sec['num_cameras'])} cameras, model of {int(model.num_cameras)}")
    dev = model.means.device
    p = sec["params"]
    n = int(p["means"].shape[0])
    for k in GAUSS_NAMES:
        old = getattr(model, k)
        new = p[k].reshape(-1, 1) if k == "opacities" else p[k]
        if int(new.shape[0]) != n or tuple(new.shape[1:]) != tuple(old.shape[1:]):
            raise ValueError(f"{k}: shape {tuple(new.shape)} in the file does not fit the model's rows {tuple(old.shape[1:])}")
        setattr(model, k, torch.nn.Parameter(new.to(device=dev, dtype=torch.float32).contiguous()))
    _fill_small(model, sec)
    model.step = int(sec["step"])
    model.radii = model.xy_grad = model.xy_absgrad = None


def _build_optimizers(model: SplatfactoDeblurModel, sec: Dict) -> Dict[str, torch.optim.Optimizer]:
    from .train_step import make_optimizers
    opts = make_optimizers(model, optimizer=sec.get("kind", "adam"))
    groups = sec["groups"]
    if set(groups) != set(opts):
        raise ValueError(f"checkpoint has optimizers {sorted(groups)}, the model needs {sorted(opts)}")
    for name, opt in opts.items():
        rec = groups[name]
        grp = opt.param_groups[0]
        grp["lr"], grp["betas"], grp["eps"] = float(rec["lr"]), tuple(float(b) for b in rec["betas"]), float(rec["eps"])
        params = grp["params"]
        if len(params) == 1:
            per_param = [(rec["step"], rec["exp_avg"], rec["exp_avg_sq"])]
        else:
            if not all(isinstance(rec[key], list) and len(rec[key]) == len(params) for key in ("step", "exp_avg", "exp_avg_sq")):
                raise ValueError(f"optimizer {name!r}: the model has {len(params)} parameters in this group, the file's "
                                 f"state does not")
            per_param = list(zip(rec["step"], rec["exp_avg"], rec["exp_avg_sq"]))
        for param, (step, exp_avg, exp_avg_sq) in zip(params, per_param):
            if step is None:
                continue
            st = {}
            for key, m in (("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
                if tuple(m.shape) != tuple(param.shape):
                    raise ValueError(f"optimizer {name!r}: {key} has shape {tuple(m.shape)}, its parameter {tuple(param.shape)}")
                st[key] = m.to(device=param.device, dtype=param.dtype).contiguous().clone()
            # fused.HipAdam counts in an int, torch.optim.Adam and train_step.SelectiveAdam in a float tensor on the CPU
            step = int(step)
            st["step"] = step if type(opt).__name__ == "HipAdam" else torch.tensor(float(step))
            opt.state[param] = st
    return opts


def _build_densify_state(sec: Dict, device, num_points: int):
    from .densify import DensifyState
    state = DensifyState(0, device, bool(sec["absgrad"]))
    for k in ("xys_grad_norm", "vis_counts", "max_2Dsize"):
        t = sec[k]
        if tuple(t.shape) != (num_points,):
            raise ValueError(f"densify_state.{k} has {tuple(t.shape)} entries, the model {num_points} rows")
        setattr(state, k, t.to(device=device, dtype=torch.float32).clone())
    state.size = (int(sec["size"][0]), int(sec["size"][1]))
    return state


def load_checkpoint(path, device="cpu", into: Optional[SplatfactoDeblurModel] = None) -> Checkpoint:
    """Read a checkpoint (torch.load(weights_only=True), never full unpickling) and build on `device`: the model at the
    saved row count with a fresh FrameHints, the optimizers through make_optimizers(model, optimizer=<saved kind>) — HipAdam
    on a GPU, torch.optim.Adam / SelectiveAdam on the CPU, whichever wrote the file — with lr / betas / eps, step counts and
    both moments filled in, the DensifyState, and the trainer / extra dicts as saved.  Sections the file does not hold
    come back as None.  A wrong format string or a newer version raises ValueError before anything is built; so do an
    unknown config key and a moment whose shape does not match its parameter.
    into: instead of building a model, restore into this one (same config and camera count; its Gaussian parameters are
    replaced by parameters of the saved row count) — `device` is then the model's."""
    obj = torch.load(os.fspath(path), map_location="cpu", weights_only=True)
    _check_header(obj)
    sec = obj["model"]
    if into is None:
        model = _build_model(sec, device)
    else:
        _restore_into(into, sec)
        model = into
    dev = model.means.device
    optimizers = None if obj.get("optimizers") is None else _build_optimizers(model, obj["optimizers"])
    dstate = None
    if obj.get("densify_state") is not None:
        dstate = _build_densify_state(obj["densify_state"], dev, model.num_points)
    return Checkpoint(model, optimizers, obj.get("trainer"), dstate, obj.get("extra"))


# --------------------------------------------------------------------------- #
# Gaussian-splat PLY
# --------------------------------------------------------------------------- #
# RECOLLECTION (no exporter in the reference tree): the vertex properties of the original 3DGS code's point_cloud.ply and
# of nerfstudio's `ns-export gaussian-splat`, all float32, in this order.  `rest` = 3 * ((sh_degree + 1)^2 - 1).
def ply_properties(rest: int) -> List[str]:
    return (["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"] + [f"f_rest_{i}" for i in range(rest)] +
            ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"])


PLY_REST_COUNTS = (0, 9, 24, 45, 72)              # sh_degree 0..4
_PLY_REQUIRED = [p for p in ply_properties(0) if p not in ("nx", "ny", "nz")]
# scalar property types of the PLY format, old and new spellings -> numpy codes (little endian)
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def ply_header(n: int, rest: int) -> bytes:
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {int(n)}"]
    lines += [f"property float {p}" for p in ply_properties(rest)]
    return ("\n".join(lines + ["end_header"]) + "\n").encode("ascii")


def export_ply(path, model: SplatfactoDeblurModel) -> int:
    """Write the model's Gaussians as a binary little-endian Gaussian-splat PLY; returns the number of rows WRITTEN.  Rows
    with any non-finite value are dropped (N minus the return value), as nerfstudio's exporter drops them.

    Values are stored as the model holds them — log-scales, opacity logits, raw (unnormalised) wxyz quaternions, SH
    coefficients — which is what the 3DGS viewers expect.  Colour convention (csrc/project.hip, gs_math.h::sh_basis): a
    Gaussian's colour is max(0.5 + sum_k B_k(dir) * sh[k], 0) with band 0 (B_0 = 0.28209...) in features_dc and the higher
    bands in features_rest, the same as the original 3DGS code.  f_rest is channel-major:
    f_rest_{c * (K-1) + k} = features_rest[n, k, c]; degree 0 writes no f_rest column.  nx ny nz are zeros.

    NOT in a PLY: camera-side parameters (pose / velocity adjustments, learnable background) and bilateral grids.  A
    model trained with rasterize_mode="antialiased" looks slightly different in a viewer that lacks the compensation
    factor (opacity scaled by sqrt(det Sigma / det (Sigma + 0.3 I)))."""
    import numpy as np
    with torch.no_grad():
        n = model.num_points
        rest = model.features_rest.detach().float().cpu()
        k1 = int(rest.shape[1])
        if 3 * k1 not in PLY_REST_COUNTS:
            raise ValueError(f"features_rest holds {k1} bands: no SH degree 0..4")
        cols = [model.means.detach().float().cpu().reshape(n, 3), torch.zeros(n, 3),
                model.features_dc.detach().float().cpu().reshape(n, 3),
                rest.permute(0, 2, 1).reshape(n, 3 * k1),                       # channel-major
                model.opacities.detach().float().cpu().reshape(n, 1),
                model.scales.detach().float().cpu().reshape(n, 3), model.quats.detach().float().cpu().reshape(n, 4)]
        table = torch.cat(cols, dim=1)
        table = table[torch.isfinite(table).all(dim=1)].contiguous()
    body = np.ascontiguousarray(table.numpy().astype("<f4")).tobytes()
    header = ply_header(table.shape[0], 3 * k1)
    _atomic_write(path, lambda f: (f.write(header), f.write(body)))
    return int(table.shape[0])


def load_ply(path) -> Dict:
    """Read a Gaussian-splat PLY (binary little endian) -> {"means" [N,3], "scales" [N,3] (log), "quats" [N,4] (wxyz,
    raw), "opacities" [N,1] (logits), "features_dc" [N,3], "features_rest" [N,K-1,3], "sh_degree"}, float32 CPU tensors
    with the values as stored.  Properties are found by NAME, in any order; other scalar properties of any standard PLY
    type are skipped.  ValueError: a format other than binary_little_endian 1.0, a missing required property, a list
    property in the vertex element, a truncated body, or a number of f_rest_* columns that is no SH degree's
    (0, 9, 24, 45, 72)."""
    import numpy as np
    with open(os.fspath(path), "rb") as f:
        raw = f.read()
    m = re.search(rb"end_header[ \t]*\r?\n", raw)
    if not raw.startswith(b"ply") or m is None:
        raise ValueError("not a PLY file (no 'ply' magic / 'end_header')")
    lines = raw[:m.start()].decode("ascii", errors="replace").splitlines()
    body = raw[m.end():]
    fmt, n, fields, element = None, None, [], None
    for ln in lines[1:]:
        t = ln.split()
        if not t or t[0] in ("comment", "obj_info"):
            continue
        if t[0] == "format":
            fmt = t[1:]
        elif t[0] == "element":
            if len(t) != 3:
                raise ValueError(f"malformed PLY header line {ln!r}")
            if n is None and t[1] != "vertex":
                raise ValueError(f"PLY element {t[1]!r} stands before the vertex element")
            element = t[1]
            if element == "vertex":
                n = int(t[2])
        elif t[0] == "property" and element == "vertex":
            if len(t) != 3 or t[1] not in _PLY_TYPES:
                raise ValueError(f"vertex property {ln!r}: only scalar properties of the standard PLY types are read")
            fields.append((t[2], "<" + _PLY_TYPES[t[1]]))
    if fmt != ["binary_little_endian", "1.0"]:
        raise ValueError(f"PLY format {' '.join(fmt or ['(none)'])!r}: only binary_little_endian 1.0 is read")
    if n is None:
        raise ValueError("PLY without a vertex element")
    names = [nm for nm, _ in fields]
    if len(set(names)) != len(names):
        raise ValueError("PLY with a repeated vertex property name")
    missing = [p for p in _PLY_REQUIRED if p not in names]
    if missing:
        raise ValueError(f"PLY misses the required properties {missing}")
    rest_ids = sorted(int(nm[len("f_rest_"):]) for nm in names if re.fullmatch(r"f_rest_\d+", nm))
    rest = len(rest_ids)
    if rest not in PLY_REST_COUNTS or rest_ids != list(range(rest)):
        raise ValueError(f"PLY with {rest} f_rest_* columns: expected f_rest_0.. with a count of {PLY_REST_COUNTS}")
    dtype = np.dtype(fields)
    if len(body) < n * dtype.itemsize:
        raise ValueError(f"truncated PLY body: {len(body)} bytes for {n} rows of {dtype.itemsize}")
    rows = np.frombuffer(body, dtype=dtype, count=n)

    def take(cols):
        if not cols:
            return torch.zeros(n, 0)
        return torch.from_numpy(np.stack([rows[c].astype(np.float32) for c in cols], axis=1))

    k1 = rest // 3
    sh_degree = PLY_REST_COUNTS.index(rest)
    return {"means": take(["x", "y", "z"]), "scales": take(["scale_0", "scale_1", "scale_2"]),
            "quats": take(["rot_0", "rot_1", "rot_2", "rot_3"]), "opacities": take(["opacity"]),
            "features_dc": take(["f_dc_0", "f_dc_1", "f_dc_2"]),
            "features_rest": take([f"f_rest_{i}" for i in range(rest)]).reshape(n, 3, k1).permute(0, 2, 1).contiguous(),
            "sh_degree": sh_degree}


def model_from_ply(path, config: Optional[SplatfactoDeblurConfig] = None, device="cpu",
                   num_cameras: int = 1) -> SplatfactoDeblurModel:
    """SplatfactoDeblurModel.from_ply: config None = the defaults at the file's SH degree; a config whose sh_degree is
    not the file's is a ValueError.  Camera-side parameters start at their initial values (they are not in a PLY)."""
    d = load_ply(path)
    if config is None:
        config = SplatfactoDeblurConfig(sh_degree=d["sh_degree"])
    elif int(config.sh_degree) != d["sh_degree"]:
        raise ValueError(f"the PLY holds SH degree {d['sh_degree']}, the config asks for {config.sh_degree}")
    model = SplatfactoDeblurModel(config, d["means"], d["scales"], d["quats"], d["opacities"], d["features_dc"],
                                  d["features_rest"], num_cameras=num_cameras)
    return model.to(device)
