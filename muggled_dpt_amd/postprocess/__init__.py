"""Depth post-processing on the GPU. Every function takes the CUDA tensor the model returned and launches HIP kernels (libmdpt: mdpt_post_*) on the
current torch stream; results stay on the device and min / max never visit the host. There is no CPU implementation: host arrays raise.
  module       functions                                                          restates (of the reference, muggled_dpt)
  display      scale_prediction, normalize_01, convert_to_uint8, pack_depth_u24,  demo_helpers/postprocess.py, toadui/colormaps.py:237-259,
               scale_and_convert_to_uint8, remove_inf_tensor, equalization_range, run_video.py:348-361, run_3dviewer.py:576-590
               threshold_bin_table, histogram_equalization, apply_colormap,
               depth_to_color, scale_prediction_images, depth_to_color_images
  still        plane_sample_points, plane_of_best_fit, depth_to_display,          run_image.py:185-195, 323-358, demo_helpers/plane_fit.py,
               depth_for_saving, depth_edge_mask, pack_depth_u24_frames           run_3dviewer.py:455-505, 576-593
  mask         depth_mask_display, depth_mask_images                              experiments/depth_masking.py
  block_norms  block_norm_display                                                 experiments/block_norm_visualization.py
  mesh         mesh_plane_grid, depth_frames_to_mesh, mesh_views                  demo_helpers/3dviewer/*.js ("Save 3D Model")
  render       render_mesh                                                        3dviewer/index.html:1158-1228 (WebGL there)
  fill         fill_holes                                                         nothing: the viewer shows the holes
  tiles        stitch_tiles                                                       nothing: results_explainer.md describes the fit
  align        fit_true_depth, depth_metrics, true_depth, mesh_depth_range        nothing: results_explainer.md describes the fit
  guided       guided_upsample_images                                             nothing: every demo resizes bilinearly
"""

from ._common import GUIDED_RECORD as _GUIDED_RECORD, PAIR_RECORD as _PAIR_RECORD, TILE_RECORD as _TILE_RECORD  # noqa: F401  (tests build tables)
from .align import ALIGN_METHODS, ALIGN_SPACES, DEPTH_METRIC_NAMES, depth_metrics, fit_true_depth, mesh_depth_range, true_depth
from .block_norms import block_norm_display
from .display import (apply_colormap, convert_to_uint8, depth_to_color, depth_to_color_images, equalization_range, histogram_equalization, normalize_01,
                      pack_depth_u24, remove_inf_tensor, scale_and_convert_to_uint8, scale_prediction, scale_prediction_images, threshold_bin_table)
from .fill import FILL_BAND, RENDER_MAX_SCRATCH_BYTES, fill_holes
from .guided import guided_upsample_images
from .mask import _size_group_batch, depth_mask_display, depth_mask_images  # noqa: F401
from .mesh import (MESH_EDGE_THRESHOLD, MESH_FOV_DEG, MESH_MAX_DEPTH, MESH_MIN_DEPTH, MESH_MODES, MESH_TARGET_FACES, depth_frames_to_mesh, mesh_plane_grid, mesh_views)
from .render import RENDER_CULL, render_mesh
from .still import (_blur_weights, depth_edge_mask, depth_for_saving, depth_to_display, pack_depth_u24_frames, plane_of_best_fit,  # noqa: F401
                    plane_sample_points)
from .tiles import TILE_ALIGN, stitch_tiles

__all__ = [name for name, value in list(globals().items()) if not name.startswith("_") and type(value).__name__ != "module"]
