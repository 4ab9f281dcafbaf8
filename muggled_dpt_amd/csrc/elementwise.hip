// HBM-bound helper kernels of the DPT path (gfx950): coalesced 8/16-byte-per-lane streaming kernels, none reshapes work into a GEMM. One
// translation unit (built once per operand format); each group's kernels and, directly below them, the mdpt_launch_* functions that launch them
// live in one ew_*.inc file (ew_common.inc first: what more than one group - and swin.hip - uses).

#include "mdpt_kernels.h"
#include "dt_io.h"
#include "up_bf16.h"
#include "ln_row.h"

#include "ew_common.inc"
#include "ew_norm.inc"     // LayerNorm (+ K-split reduction), K-split finish, per-token norm, SwiGLU, weight-rounding compensation
#include "ew_tokens.inc"   // patchify, NaN poison, position-embedding resize, cls / pad rows, token import / export, BEiT relative position tables
#include "ew_resize.inc"   // bilinear (align_corners) upsample: direct, LDS-tiled, bf16 -> bf16
#include "ew_pack.inc"     // one-time weight repack (16-bit and fp8 planes, power-of-two scale), padded copy, fill, add
#include "ew_layout.inc"   // NCHW <-> NHWC conversion of the stage-level API
#include "ew_prepare.inc"  // uint8 BGR frame -> normalised model tensor (antialiased resize), alone and fused with patchify
