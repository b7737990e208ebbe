"""3dgs-deblur_amd — MI355X-native differentiable 3DGS rasterizer with motion-blur /
rolling-shutter sub-frame averaging (the one hot path of SpectacularAI/3dgs-deblur).

The directory name is not a valid Python identifier; import it as ``gsdeblur_amd``
(the repo-root shim ``gsdeblur_amd.py`` registers this package under that name).
"""
from . import _lib  # noqa: F401
from .ops import (  # noqa: F401
    project_gaussians,
    rasterize_gaussians,
    spherical_harmonics,
    map_gaussian_to_intersects,
    get_tile_bin_edges,
    compute_cumulative_intersects,
    bin_and_sort_gaussians,
    bin_and_sort_records,
    render_subposes,
    render_combined,
    render_batch,
    subpose_viewmats,
    subpose_schedule,
    subpose_times,
    combine_samples,
    exclusive_scan_u32,
    radix_sort_pairs,
)
from .model import Camera, CameraShutterOptimizerConfig, SplatfactoDeblurConfig, SplatfactoDeblurModel  # noqa: F401
from . import dp  # noqa: F401
from . import bilagrid, blurscore, checkpoint, colorcorrect, data, densify, depthprior, fused, mcmc, normals, step, train_step as training, tsdf  # noqa: F401
from .colorcorrect import color_correct  # noqa: F401
from .depthprior import depth_prior_loss, depth_prior_loss_with_grad  # noqa: F401
from .knn import knn, knn_mean_distance  # noqa: F401
from .tsdf import TSDFVolume, tsdf_integrate, tsdf_extract_mesh  # noqa: F401
from . import meshclean  # noqa: F401
from .meshclean import mesh_components, mesh_filter_components  # noqa: F401
from . import meshdecimate  # noqa: F401
from .meshdecimate import mesh_decimate  # noqa: F401
from .normals import depth_normals, normal_loss, normal_loss_with_grad  # noqa: F401
from .blurscore import blur_stats  # noqa: F401
from .step import render_step  # noqa: F401
from .data import load_transforms, load_seed_points_ply  # noqa: F401

__version__ = "0.1.0"
