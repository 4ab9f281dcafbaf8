// Depth post-processing on the GPU: everything that happens to a depth map after the DPT forward, without a host round trip of the full-resolution
// fp32 map. One translation unit; each feature's kernels and, directly below them, the mdpt_launch_post_* functions that launch them live in one
// post_*.inc file, included in dependency order (post_common.inc first: what more than one feature uses).

#include "mdpt_kernels.h"
#include "dt_io.h"
#include "mdpt_prof.h"

#include "post_common.inc"
#include "post_display.inc"  // min/max, scale, normalize, the per-image display tail, equalize, colorize, block-norm tiles
#include "post_still.inc"    // plane fit / removal, threshold display, edge alpha, 24-bit packing, depth masks and cutouts
#include "post_mesh.inc"     // depth-to-mesh export
#include "post_tiles.inc"    // tiled high-resolution inference: fit to a guide, feather blend
#include "post_align.inc"    // true-depth alignment to ground truth, metrics
#include "post_guided.inc"   // photo-guided upsampling
#include "post_render.inc"   // rendering of depth meshes
#include "post_fill.inc"     // hole filling of rendered views
#include "post_video.inc"    // temporally stable video depth: frame-to-frame fit, temporal filter, carried display range
#include "post_refocus.inc"  // synthetic depth of field: per-pixel defocus, occlusion-aware LDS-tiled gather
#include "post_normals.inc"  // surface normals and relighting: edge-aware differences of the unprojected map over an LDS tile, V lights a pass
#include "post_shadows.inc"  // cast shadows and ambient occlusion for the relighting: marches over an LDS tile of a working grid, folded into the shading
#include "post_segment.inc"  // depth segmentation: union-find over LDS tiles, lock-free merge across tiles, region tables, pick-to-cutout
#include "post_localfit.inc" // locally varying true-depth alignment: moments per grid cell, window fits, a coefficient field applied per pixel
