// Internal kernel-launcher interface of libmdpt (gfx950 only). Not part of the public C ABI
// (that is include/mdpt.h); this header is shared by the .hip kernel files and the host-side files (mdpt_internal.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "op_types.h"

// element types of tensors that cross the C ABI (= MDPT_DTYPE_* of include/mdpt.h)
enum { MDPT_DT_F32 = 0, MDPT_DT_BF16 = 1, MDPT_DT_F16 = 2 };

// ------------------------------------------------------------------------------------------------
// GEMM / implicit-GEMM convolution family:  C[M,N] = A[M,K] * W[N,K]^T   (both operands K-contiguous)
// A and W are bf16 "hi" planes plus optional "lo" planes (x = hi + lo, bf16x3 split precision).
// ------------------------------------------------------------------------------------------------
enum { MDPT_A_DENSE = 0, MDPT_A_TOKENS = 1, MDPT_A_CONV3 = 2 };
enum { MDPT_E_GENERIC = 0, MDPT_E_QKV = 1, MDPT_E_PATCH = 2, MDPT_E_D2S = 3, MDPT_E_HEAD = 4, MDPT_E_SWQKV = 5 };
enum { MDPT_ACT_NONE = 0, MDPT_ACT_RELU = 1, MDPT_ACT_GELU = 2 };
enum { MDPT_TILE_AUTO = 0, MDPT_TILE_128x128 = 1, MDPT_TILE_256x256 = 2, MDPT_TILE_128x32 = 3, MDPT_TILE_256x128 = 4, MDPT_TILE_PP256 = 5, MDPT_TILE_64x64 = 6 };

struct GemmParams {
    // operands
    const op_t* A_hi; const op_t* A_lo;   // activations, row stride lda (elements)
    const op_t* W_hi; const op_t* W_lo;   // weights [N][K]
    int M, N, K;                              // K % 64 == 0 (conv: K = 9 * Cin)
    int ldw;                                  // row stride of W in elements (0 = K: the packed panels; > K: a K range of wider rows, see ksplit)
    int M_alg;                                // > 0: rows that are algorithmic work (token rows without the per-image pad rows): profiler FLOP accounting only
    int lda;
    int npass;                                // 1 = one rounded plane per operand, 3 = split planes (A_lo*W_hi + A_hi*W_lo + A_hi*W_hi),
                                              // 2 = activations split, weights one plane (A_lo*W_hi + A_hi*W_hi)
    const op_t* zero_page;                  // >= 256 B of zeros (source for padded conv taps)
    int amode, ekind, tile;
    // A_TOKENS: logical row m = (b, p) reads source row b*tok_stride + 1 + p (skips the cls row)
    int tok_np, tok_stride;
    // A_CONV3: input NHWC [B,Hi,Wi,Cin] (Cin % 64 == 0), 3x3, pad 1, stride cstride -> [B,Ho,Wo,N]
    int Hi, Wi, Cin, Ho, Wo, cstride;
    // generic epilogue: v = acc (+bias[n]) -> act -> (*gamma[n]) (+resid[m,n]) (+up2x(up_src)[m,n])
    const float* bias; const float* gamma; const float* resid; int ldr;
    int bias_img_stride, bias_img_rows;       // stride != 0: `bias` is a table, row m uses bias + (m / bias_img_rows) * bias_img_stride (per-image
                                              // bias: BEiT readout cls term; token-mean compensation of the weight rounding in the fp16 modes)
    const float* up_src; int Hu, Wu;          // fp32 NHWC [B,Hu,Wu,N] added through x2 bilinear (align_corners)
    int act;
    float* out_f32; op_t* out_hi; op_t* out_lo; int ldc;
    int relu_bf16;                            // apply ReLU to the bf16 planes only (fp32 copy stays raw)
    int acc_init;                             // 1: accumulators start at resid[m,n] (resid == out_f32, gamma folded into W / bias): out = (resid + A W^T) + bias
    const float* wscale;                      // fp16 build, generic epilogue: device {s, 1 / s}, s a power of two the packed weight planes were multiplied by (the
                                              // layer-scale-folded matrices, mdpt_launch_weight_scale): accumulators start at resid * s, v = acc * (1 / s) (+ bias ...)
                                              // - exact rescalings, so the planes' lo halves stay out of fp16's subnormal range whatever gamma is. null = 1
    // E_QKV: scatter to head-major Q (pre-scaled), K and transposed V
    op_t* q_hi; op_t* q_lo; op_t* k_hi; op_t* k_lo; op_t* vt_hi; op_t* vt_lo;
    int F, heads, npad, npadv; float qscale;
    // E_SWQKV, the SwinV2 QKV projection (its own kernel; 8-phase tile only, 2F % 256 == 0): Q / K column tiles are written as the window
    // attention's operands - q / max(|q|, 1e-12) * logit_scale[h], k / max(|k|, 1e-12), heads of 32, row (img*swin_img_rows +
    // swin_tokmap[t] + h*npad) for image token t - and V column tiles as fp32 into out_f32 (ldc = 3F) for swin_v_prep
    const int* swin_tokmap; const float* swin_logit_scale; int swin_N, swin_img_rows;
    // ... and, when swin_vtokmap != nullptr (token runs of 4 stay together: gw, ww, shift % 4 == 0), the V column tiles are written as the
    // transposed window operand Vt[(img*nw + w)*heads + h][d][npadv] directly: element img*swin_img_velems + swin_vtokmap[t] + (h*32 + d)*npadv
    const int* swin_vtokmap; int swin_img_velems;
    // E_PATCH: out_f32[(b*npad + 1 + p), n] = acc + bias[n] + pos[p, n]   (m = b*tok_np + p)
    const float* pos;
    // E_D2S: transposed conv k==s as GEMM: n = (ky*k + kx)*Cout + co ; out NHWC [B, Ho*k, Wo*k, Cout]
    int d2s_k, d2s_cout;
    // E_HEAD: N == 32: depth[m] = final( sum_n relu(acc+bias[n]) * head_w[n] + head_b )
    const float* head_w; const float* head_b; int head_sigmoid; void* head_out; int head_out_dtype;  // MDPT_DT_*
    // test hook: per-workgroup phase timestamps (s_memtime): [start, first barrier passed, main loop done, epilogue done]
    int throughput_mode;  // 1: another stream runs the other half batch concurrently -> pick tiles by CU-time efficiency, not latency
    // K split: ksplit > 1 splits K into ksplit equal ranges, one workgroup each (grid.y). Range 0 runs the normal epilogue; range z >= 1 stores its
    // bare fp32 partial sums to ks_part + (z - 1) * M * ldc, and the CONSUMER adds them in the order z = 1, 2, ... - the LayerNorm that follows
    // (mdpt_launch_layernorm_addp, mdpt_launch_ln_res). A fixed split: bits do not depend on the batch. Two users:
    //  * latency mode, proj / fc2 of a small batch (one 16 ... 64-K-tile serial chain per 64x64 workgroup): dense A, generic epilogue, 64x64 tile
    //    (four ranges on the 128x128 tile - half the operand traffic per flop - measured 7 % slower: profiles/r04_b1_ksplit_sweep.txt);
    //  * SwinV2 fc2 with K >= 3072 at EVERY batch size (stages of few, long-K tiles: 108 8-phase tiles at batch 16): fp32 output without
    //    residual (DM_F32 form of the 8-phase kernel from 140 workgroups on, the 64x64 tile below - same sums, same bits).
    // fp8 cross terms (f8_cross.h, fp16 build; npass 2 or 3): f8 != 0 -> A_lo points at the e5m2 RESIDUE plane of the activations (bytes, rows of lda
    // bytes) and the cross terms run on the block-scaled MFMA: A_lo8 W8^T, then (npass == 3) A8 W8_lo^T with the e5m2 plane of the values at
    // (bytes) A_lo + a8_off, then A_hi W_hi^T on the fp16 planes. K % 128 == 0; conv K order of the fp8 planes: k = (cb128 * 9 + tap) * 128 + c.
    int f8; size_t a8_off;
    const unsigned char* W8; const unsigned char* W8_lo;   // [N][K] e4m3 bytes (row stride K)
    const unsigned char* S8; const unsigned char* S8_lo;   // [N] E8M0 bytes: power-of-two scale of every weight row
    // output planes for an F8 consumer: out_f8 != 0 -> out_lo receives BYTES: the e5m2 residue plane (element index = out_hi's) and, out_a8 != 0,
    // the e5m2 plane of the values themselves at byte offset out_f8 (= the plane's element count)
    size_t out_f8; int out_a8;
    int ksplit; float* ks_part;
    int ks_all;  // 1: EVERY range (z = 0 too) stores its bare partial sums, plane z at ks_part + z * M * ldc, and nothing else is written: a finishing
                 // kernel (mdpt_launch_ksplit_finish) adds the planes in the order z = 0, 1, ... and applies bias / ReLU / the output planes.
                 // Dense rows or 3x3-conv rows, 64x64 tile. Latency mode: the long-K convs of the 18^2 / 36^2 levels at batch 1.
    // test hook: six 64-bit slots per workgroup, written by stamp_record (mfma_common.inc): clock stamps [start, first barrier, loop done, stores
    // acknowledged], then by epilogue  LDS strip (both kernels): [XCC id, HW_REG_HW_ID];  direct: [stores issued, HW_REG_HW_ID];
    // transposed V: [stores acknowledged again, 0]
    unsigned long long* dbg_times;
};


// ------------------------------------------------------------------------------------------------
// halo-staged 3x3 convolution, stride 1, pad 1, Cout = 256 (conv3h.hip): the 256-channel convs of the DPT decoder at large batch.
//   out = ((conv3x3(in) [+ bias]) [+ x2 bilinear (align_corners) of up_src]) [+ skip]  ->  out_f32 (optional) and out_bf (ReLU'd if relu_bf)
// Same K order (MDPT_PACK_CONV3 weights) and epilogue arithmetic as the MDPT_A_CONV3 path of mdpt_launch_gemm (generic epilogue, resid = skip).
// ------------------------------------------------------------------------------------------------
struct Conv3hParams {
    const op_t* in;          // NHWC [B, H, W, Cin] bf16 (hi plane), Cin % 128 == 0
    const op_t* up_in; int Hs, Ws;  // instead of `in` (Cout = 128, bf16 only): bf16 NHWC [B, Hs, Ws, Cin]; the conv input is its bilinear
                               // (align_corners) upsample to H x W, interpolated inside the kernel (up_bf16.h arithmetic)
    const op_t* in_lo;       // lo plane of the input: non-null selects the bf16x3 mode (then w_lo and, with out_bf, out_bf_lo are required)
    const op_t* w;           // [Cout][9 * Cin] bf16, MDPT_PACK_CONV3 order (hi plane)
    const op_t* w_lo;
    const float* bias;         // [Cout] or null
    const float* skip;         // fp32 NHWC [B, H, W, 256] or null
    const float* up_src; int Hu, Wu;  // fp32 NHWC [B, Hu, Wu, 256] or null
    float* out_f32;            // fp32 NHWC [B, H, W, 256] or null
    op_t* out_bf;            // bf16 NHWC [B, H, W, Cout] (hi plane); Cout = 128 may write the fp32 map alone instead
    op_t* out_bf_lo;
    int relu_bf;
    int B, H, W, Cin;
    int Cout;                  // 256 (every epilogue form) or 128 (bias-only bf16 output: the head's first conv)
    // fp8 cross terms (GemmParams::f8 has the description): in_lo = e5m2 residue plane (bytes, NHWC), values' plane at in_lo + a8_off (three terms:
    // w8_lo != null), weights [Cout][9 * Cin] e4m3 bytes in 128-channel-block K order + per-row E8M0 scales; output planes as GemmParams::out_f8
    int f8; size_t a8_off;
    const unsigned char* w8; const unsigned char* w8_lo; const unsigned char* s8; const unsigned char* s8_lo;
    size_t out_f8; int out_a8;
    unsigned long long* dbg_times;  // test hook: the six-slot record of GemmParams::dbg_times in the layout [start, first barrier, loop done, stores acknowledged, stores issued, XCC id]
};

// ------------------------------------------------------------------------------------------------
// fused multi-head attention (head dim 64), Q/K head-major [B,H,npad,64], Vt [B,H,64,npadv]
// ------------------------------------------------------------------------------------------------
struct AttnParams {
    const op_t* q_hi; const op_t* q_lo; const op_t* k_hi; const op_t* k_lo;
    const op_t* vt_hi; const op_t* vt_lo;
    op_t* out_hi; op_t* out_lo;           // [B*npad, F] token-major, column h*64 + d
    int B, heads, N, npad, npadv, F;
    int x3;
    // additive relative-position bias (BEiT): per-head extended LUT [heads][bias_elen] fp32, s[q][k] += lut[tq[q] - tk[k]]
    const float* bias_lut; int bias_elen; const int* tq; const int* tk;
    // SwinV2 window attention (rowmap != null): head_dim 32, B = images * win_nw windows of N tokens each,
    // rowmap[win_nw*N] = image token of every window token, region[win_nw][region_ld] = shifted-window region ids (null: no mask)
    int head_dim;  // 0 = 64
    int win_nw; const int* rowmap; const int* region; int region_ld;
    int bias_run4;       // window width and tokens per window are multiples of 4: four consecutive keys have consecutive bias-table indices
    int bias_row;        // (bias_run4) row length 2 ww - 1 of the table and window width ww: the LDS image of the table is re-strided so that 32
    int bias_ww;         // consecutive query tokens read 32 different banks (attention.hip, round 6); 0 = the table's own row length
    const float* swin_ls; // (window attention) the packed logit scale per head = exp(clamped logit_scale) * log2(e): Q carries it, the kernel's fixed softmax
                          // reference point is built from it (attention.hip FIXREF)
    int out_ld;          // row stride of out_hi / out_lo in elements (0 = F); pad columns are the caller's
    int allow_split_kv;  // latency mode: small launches may split the key loop over the waves (not batch-invariant in the last bit)
    int tail_last;  // set by the launcher: dispatch nearly empty last q-tiles after all full ones
};

// ------------------------------------------------------------------------------------------------
// bandwidth-bound helpers
// ------------------------------------------------------------------------------------------------
// weight repack: source (fp32 / bf16 / fp16: src_dtype) in PyTorch layout -> bf16 hi (+lo) [Np][Kp] rows, zero padded. Layout kinds:
enum { MDPT_PACK_LINEAR = 0,   // src [N][K]
       MDPT_PACK_CONV3 = 1,    // src [Cout][Cin][3][3] -> k = (cb*9 + ky*3+kx)*64 + c, ci = cb*64 + c (64-channel block outer, tap inner)
       MDPT_PACK_CONVT = 2,    // src [Cin][Cout][k][k] -> row n = (ky*k+kx)*Coutp + co, col ci
       MDPT_PACK_CONV3_KC32 = 3 };  // src [32][Cin][3][3] -> [Kp/8][32][8] (k = (ky*3+kx)*Cinp + ci in 8-element chunks, Np = 32): the
                                    // LDS image of head_tail_kernel, where a 32-lane fragment read is 512 consecutive bytes
struct BeitRelposBatch {
    const float* ref[32]; float* ext0; size_t ext_stride;  // block l writes ext0 + l * ext_stride (elements)
    int* tq; int* tk;
    int n, heads, Gh, Gw, gh, gw, N, ntok_pad;
};

// ------------------------------------------------------------------------------------------------
// fused tail of the depth head (head.hip): x(P/8) bilinear upsample -> 3x3 conv (cin -> 32) + ReLU -> 1x1 (32 -> 1) + ReLU | sigmoid
// ------------------------------------------------------------------------------------------------
struct HeadTailParams {
    const op_t* src;    // [B, Hi, Wi, cin] bf16 NHWC: output of the head's first conv (pad channels zero)
    const op_t* src_lo; // lo plane of the same map (src = hi): non-null selects the two-pass form (activations split, weights one plane)
    const op_t* w_kc;   // MDPT_PACK_CONV3_KC32 image of the 3x3 conv weights
    const float* bias;    // [32]
    const float* head_w;  // [32] 1x1 conv weights
    const float* head_b;  // [1]
    void* out; int out_dtype;  // depth [B, Ho, Wo], MDPT_DT_*
    int sigmoid;
    int B, Hi, Wi, Ho, Wo;
    unsigned long long* dbg_times;  // test hook (MDPT_HEAD_DBG=1): per-workgroup s_memtime stamps of the phases of its 2nd tile
};

// ------------------------------------------------------------------------------------------------
// SwinV2 helpers (swin.hip)
// ------------------------------------------------------------------------------------------------
// frame table of the fused resize + normalise + im2col kernel (prepare_patchify_kernel), passed BY VALUE as a kernel argument (nothing is
// copied to the device, so a forward from uint8 frames stays graph-capturable): run r holds `count` uint8 [ih,iw,3] frames from `ptr`, each read
// where it lies: rows `pitch` bytes apart, frame j at ptr + j frame_stride (bytes). Packed frames have pitch = 3 iw and frame_stride = 3 ih iw; a
// box of an image is a frame whose ptr is the box's first pixel, ih x iw the box's size and pitch the IMAGE's row pitch.
// The frames of a launch are the runs' frames in order (blockIdx.y = frame); one size for the whole batch is one run (also one box cut out of
// every frame of a [B,H,W,3] tensor), a list of frames or boxes of different sizes is one run per frame. 64 runs = 2.5 KB of kernel arguments.
#define MDPT_BGR_RUNS 64
struct BgrRun { const unsigned char* ptr; long long pitch, frame_stride; int ih, iw, count; };
struct BgrRunTable { BgrRun run[MDPT_BGR_RUNS]; int n; };
// HIP passes at most 4 KB of kernel arguments: the table plus the other arguments of prepare_patchify_kernel (two pointers, five ints, six floats)
static_assert(sizeof(BgrRunTable) <= 3072, "BgrRunTable must leave room for the other kernel arguments below HIP's 4 KB limit");

// image table of the per-image display tail (post_display.inc seg_* and colorize kernels), by value like BgrRunTable: run r holds `count`
// packed images of ih x iw elements from `in` (image j at in + j ih iw) whose outputs are oh x ow (the resize target; = ih x iw for the
// kernels that do not resize) and start at element `off` of the packed output (image j at off + j oh ow). The images of a launch are the
// runs' images in order (blockIdx.y = image); a uniform batch is one run.
#define MDPT_POST_RUNS 32
struct PostRun { const void* in; size_t off; int ih, iw, oh, ow, count; };
struct PostRunTable { PostRun run[MDPT_POST_RUNS]; int n; };

// the one-run image table of a uniform batch: B images of ih x iw (-> oh x ow) packed from `in`, outputs packed from element 0
inline PostRunTable uniform_table(const void* in, int B, int ih, int iw, int oh, int ow) {
    PostRunTable t{};
    t.n = 1;
    t.run[0] = PostRun{in, 0, ih, iw, oh, ow, B};
    return t;
}

// a prepared uniform batch of the still-image display tail with its statistics, by value: maps [B, h, w] of dtype dt from `in`, parts = [B,
// MDPT_POST_SEG_PARTS, 2] ordered {min, max} partials, coef = [B, 4] fp64 plane {nx, ny, nz, d}, factor = the share of the plane to remove, vparts =
// [B, MDPT_POST_SEG_PARTS, 2] fp64 {min, max} partials of the plane-removed map (null for the kernel that computes them)
struct PlaneMap { const void* in; int dt, B, h, w; const unsigned* parts; const double* coef; double factor; const double* vparts; };

// photo table of the depth-masking cutout (post_still.inc mask_cutout_kernel), by value: photo k is img (ih x iw x 3 BGR bytes), cut out by its
// prepared map (h x w, dtype dt of the table) with that map's min/max partials, plane coef and plane-removed min/max partials; its outputs start at
// pixel `off` of the packed BGRA / mask outputs (blockIdx.y = photo)
#define MDPT_MASK_IMAGES 32
struct MaskImage { const void* map; const unsigned* parts; const double* coef; const double* vparts; const unsigned char* img; size_t off; int h, w, ih, iw; };
struct MaskTable { MaskImage im[MDPT_MASK_IMAGES]; int n, dt; };

// one depth-to-mesh call (post_mesh.inc mesh_* kernels), by value: B frames [H, W, 4] of 24-bit depth + alpha bytes, a plane grid of nx x ny
// vertices (vertex i = c + r nx at (c x_step - 1, 1 - r y_step), or at vertex_xy[i] when the fp64 [nx ny, 2] table is given), the camera of the
// viewer's vertex shader (depth = a + b d, or 1 / (a + b d) for relative models; alpha_min = edge_threshold * 255) and the scratch planes of the
// multi-launch compaction: vmap [B, nx ny] (-1 = dropped vertex, else its new index), vcnt / fcnt = per-block kept counts -> exclusive offsets,
// bord [B, 6] ordered-uint {min xyz, max xyz}
struct MeshJob {
    const unsigned* frames; const double* vertex_xy;
    int B, H, W, nx, ny, is_metric, points;
    double x_step, y_step, a, b, tan_half_fov, x_scale, y_scale, alpha_min;
    int* vmap; unsigned* vcnt; unsigned* fcnt; unsigned* bord;
};
inline size_t mesh_blocks(size_t n) { return (n + 255) / 256; }  // the compaction's blocks: 256 vertices (or grid cells) each

// one render call (post_render.inc render_* kernels), by value: the slabs of mdpt_launch_post_mesh read in place (xyz [B, nv, 3], uv [B, nv, 2], faces
// [B, nf, 3] or, for points, [B, nf = nv, 1], counts [B, 2] on the device), one texture per mesh (tex: B RenderTex records in DEVICE memory, =
// mdpt_texture of include/mdpt.h), view_proj fp64 [B, V, 16] (clip = [x, y, z, 1] M), the H x W viewport, half = the points' half-size in 1/256
// pixel, and the scratch: verts [B V, nv] transformed vertices, zbuf [B V, H W] keys
struct RenderTex { const unsigned char* bgr; int h, w; };
struct RenderVertex { int x, y; double invw, z01; };  // snapped screen position (x == RENDER_UNUSABLE: w <= 0 or off the fixed-point range)
#define RENDER_UNUSABLE (-2147483647 - 1)
#define RENDER_SMALL_BOX 64    // a face whose clipped box holds at most this many pixels is walked by its own lane, a larger one by its workgroup
#define RENDER_MAX_SIDE 32768  // of the viewport: pixel centres stay below 2^23 in 1/256 pixel
struct RenderJob {
    const float* xyz; const float* uv; const int* faces; const int* counts; const RenderTex* tex; const double* view_proj;
    int B, V, nv, nf, H, W, points, cull_back, half;
    RenderVertex* verts; unsigned long long* zbuf;
};
inline size_t render_scratch_bytes(size_t B, size_t V, size_t nv, size_t H, size_t W) { return B * V * (nv * sizeof(RenderVertex) + H * W * 8); }

// hole filling of rendered views (post_fill.inc fill_* kernels): the push-pull pyramid of N images of H x W. Level 0 is the image, level l has
// ceil(H / 2^l) x ceil(W / 2^l) nodes up to the 1 x 1 level L; a node = 16 bytes {three colour channels, depth} fp32, depth 0 = invalid. The scratch
// holds levels 1 .. L of every image, image after image, level after level; top = the first level of at most FILL_TOP_SIDE nodes a side.
#define FILL_TOP_SIDE 32    // levels of at most this many nodes a side are one workgroup's, in LDS
#define FILL_PUSH_LEVELS 3  // a push workgroup owns an aligned 32 x 32 block of its base level and makes up to this many levels above it
#define FILL_MAX_LEVELS 16  // sides of at most RENDER_MAX_SIDE = 2^15: L <= 15
__host__ __device__ inline int fill_level_side(int side, int l) { return (int)(((long long)side + (1ll << l) - 1) >> l); }
struct FillPlan {
    int H, W, L, top;
    size_t off[FILL_MAX_LEVELS + 1];  // off[l] = level l's first node within an image's scratch (l >= 1); off[L + 1] = the nodes of one image
};
inline FillPlan fill_plan(int H, int W) {
    FillPlan p{};
    p.H = H, p.W = W, p.top = -1;
    size_t at = 0;
    for (int l = 0;; ++l) {
        const int h = fill_level_side(H, l), w = fill_level_side(W, l);
        if (p.top < 0 && h <= FILL_TOP_SIDE && w <= FILL_TOP_SIDE) p.top = l;
        p.off[l] = at;
        if (l >= 1) at += (size_t)h * w;
        if (h == 1 && w == 1) {
            p.L = l;
            break;
        }
    }
    p.off[p.L + 1] = at;
    return p;
}
inline size_t fill_scratch_bytes(size_t N, int H, int W) {
    const FillPlan p = fill_plan(H, W);
    return N * (p.off[p.L + 1] ? p.off[p.L + 1] : 1) * 16;  // (a 1 x 1 image has no level above it: one node, never touched)
}
struct FillJob {
    const unsigned char* color; const float* depth; unsigned char* out; float* out_depth; void* scratch;
    int N; double keep;  // keep = 1 - band
    FillPlan plan;
};

// one tile of tiled high-resolution inference (post_tiles.inc tile_* kernels; = mdpt_tile of include/mdpt.h): its h x w map (the table's dtype) and
// its half-open pixel box in the photo. The table lives in DEVICE memory (any number of tiles); the kernels index it by tile.
struct PostTile { const void* map; int h, w, x1, y1, x2, y2; };
// samples of one tile map that one workgroup of the fit reduces (256 threads x 8): the partial sums of tile t's chunk c are the 6 doubles at
// parts[(t max_chunks + c) 6], max_chunks = the chunks of the call's largest map
#define MDPT_TILE_FIT_CHUNK 2048
__host__ __device__ inline size_t tile_fit_chunks(size_t map_elems) { return (map_elems + MDPT_TILE_FIT_CHUNK - 1) / MDPT_TILE_FIT_CHUNK; }

// one prediction / ground-truth pair of the true-depth block (post_align.inc align_* kernels; = mdpt_depth_pair of include/mdpt.h): the ph x pw
// prediction (the table's dtype), the H x W fp32 truth and its uint8 validity map (null: every pixel). Device table, indexed by pair; apply reads
// pred, ph, pw and H x W (its output size) only.
struct AlignPair { const void* pred; int ph, pw; const float* truth; const unsigned char* valid; int H, W; };
#define ALIGN_METRIC_SUMS 11   // = MDPT_ALIGN_NUM_METRICS: the partial sums of a chunk and the metrics of a pair
#define ALIGN_HIST_WORDS 1024  // the radix select's bins of a pair: [2 streams][2 rank tracks][256 digits]
#define ALIGN_STATE_WORDS 16   // its state: 4 prefixes, 4 ranks, n
#define ALIGN_STRIDE_BLOCKS 1024 // workgroups a pair's grid-stride passes (the select's histogram, apply) are spread over, at most
// ... for a call whose largest map has max_pixels pixels: one per 2048 pixels, capped
inline int align_stride_blocks(size_t max_pixels) {
    const size_t b = (max_pixels + 2047) / 2048;
    return (int)(b < 1 ? 1 : (b > ALIGN_STRIDE_BLOCKS ? ALIGN_STRIDE_BLOCKS : b));
}
// the scratch of a table of P pairs whose largest truth has max_chunks chunks of MDPT_TILE_FIT_CHUNK pixels: [P, max_chunks, ALIGN_METRIC_SUMS]
// fp64 partials (the fits use the front of it), then the select's bins and state
inline size_t align_parts_doubles(size_t P, size_t max_chunks) { return P * max_chunks * ALIGN_METRIC_SUMS; }
inline size_t align_scratch_bytes(size_t P, size_t max_chunks) {
    return align_parts_doubles(P, max_chunks) * sizeof(double) + P * (ALIGN_HIST_WORDS + ALIGN_STATE_WORDS) * sizeof(unsigned);
}

// one map / photo pair of the photo-guided upsampling (post_guided.inc guided_* kernels; = mdpt_guided_pair of include/mdpt.h): the h x w map (the
// table's dtype), the uint8 BGR photo of H x W pixels whose rows lie `pitch` bytes apart (any alignment), the fp32 H x W output, and where the pair's
// scratch starts (bytes from the call's scratch pointer, a multiple of 8). Device table, indexed by pair.
struct GuidedPair { const void* map; int h, w; const unsigned char* photo; long long pitch; int H, W; float* out; long long scratch_off; };
#define GUIDED_MAX_RADIUS 64
#define GUIDED_MOMENTS 13  // window sums of a cell: g (3), g g^T (6: BB BG BR GG GR RR), p, g p (3)
// a pair's scratch in 8-byte words per cell: the integer cell sums {n, SB, SG, SR}, the coefficients {aB, aG, aR, b} as four planes, their window means
// interleaved [h, w, 4], and the row sums of whichever window pass is running (13 planes, the coefficient pass uses the first 4)
#define GUIDED_WORDS_PER_CELL (4 + 4 + 4 + GUIDED_MOMENTS)
inline size_t guided_pair_scratch_bytes(size_t h, size_t w) { return h * w * GUIDED_WORDS_PER_CELL * 8; }

// the same for every block of the encoder in ONE launch (the LUTs depend on weights and window sizes only, not on activations)
struct SwinCpbBatch {
    const float* w1[32]; const float* b1[32]; const float* w2[32]; float* lut[32];
    int heads[32], wh[32], ww[32], pre[32];
    int n, hidden;
};

// ------------------------------------------------------------------------------------------------
// depth post-processing (postprocess.hip: the post_*.inc files, each launcher below its kernels); scratch2 = 2 uints of device scratch for the min/max reduction
// ------------------------------------------------------------------------------------------------
int mdpt_launch_post_minmax(const float* in, size_t n, float* minmax_out, unsigned* scratch2, hipStream_t stream);
int mdpt_launch_post_scale(const float* in, float* out, int B, int ih, int iw, int oh, int ow, float* minmax_out,
                           unsigned* scratch2, hipStream_t stream);
int mdpt_launch_post_normalize(const float* in, const float* minmax, void* out, size_t n, int mode, int lossy,
                               hipStream_t stream);
// per-image display tail: parts = [B, MDPT_POST_SEG_PARTS, 2] ordered {min, max} partials, hist / hist_clear = [B, 256] counts, lut = [B, 256],
// B = the table's images (every per-image buffer starts at the table's first image); out (fp32 / uint8) is the packed output of PostRun::off
int mdpt_launch_post_seg_minmax(const PostRunTable& t, int in_dt, float* out, unsigned* parts, unsigned* hist_clear, hipStream_t stream);
int mdpt_launch_post_seg_u8(const PostRunTable& t, int in_dt, const unsigned* parts, int reverse, unsigned char* out, unsigned* hist,
                            hipStream_t stream);
int mdpt_launch_post_hist(const unsigned char* in, int B, size_t n, unsigned* hist, hipStream_t stream);
int mdpt_launch_post_eq_lut(const unsigned* hist, int B, const int* bin_of, int vmin, int vmax, unsigned char* lut, hipStream_t stream);
int mdpt_launch_post_colorize(const PostRunTable& t, const unsigned char* eq, const unsigned char* cmap, int channels, unsigned char* out,
                              hipStream_t stream);
// still-image display tail and edge alpha (uniform batches): PlaneMap above, mag = [B, h, w] fp32 Sobel magnitude, mag_max = [B] fp32 bits (cleared
// by the edge launcher)
int mdpt_launch_post_display_prep(const void* in, int dt, int B, int ih, int iw, void* out, int oh, int ow, unsigned* parts, unsigned* hist_clear,
                                  hipStream_t stream);
int mdpt_launch_post_plane_fit(const void* in, int dt, int B, int h, int w, const unsigned* parts, const int* xy, int N, size_t xy_stride, double* coef,
                               hipStream_t stream);
int mdpt_launch_post_plane_eval(const double* coef, int B, int h, int w, float* out, hipStream_t stream);
int mdpt_launch_post_plane_minmax(const PlaneMap& m, double* vparts, hipStream_t stream);
int mdpt_launch_post_threshold(const PlaneMap& m, double tmin, double delta, int mode, int reverse, void* out, unsigned* hist, hipStream_t stream);
int mdpt_launch_post_edge_mag(const float* in, int B, int h, int w, const unsigned* parts, const float* blur_w, int ksize, float* mag, unsigned* mag_max,
                              hipStream_t stream);
int mdpt_launch_post_edge_mask(const float* mag, const unsigned* mag_max, int B, size_t n, unsigned char* out, hipStream_t stream);
int mdpt_launch_post_pack_u24(const float* in, int B, size_t n, const unsigned* parts, int lossy, const float* mag, const unsigned* mag_max,
                              const unsigned char* mask, size_t mask_stride, unsigned char* out, hipStream_t stream);
// depth masking (experiments/depth_masking.py): the display mask + checker composite of a uniform batch (images [B, ih, iw, 3]) and the
// per-photo cutout at each photo's own size
int mdpt_launch_post_mask_display(const PlaneMap& m, double tmin, double tmax, int invert, const unsigned char* img, int ih, int iw, unsigned char* mask,
                                  unsigned char* comp, hipStream_t stream);
int mdpt_launch_post_mask_cutout(const MaskTable& t, double factor, double tmin, double tmax, int invert, unsigned char* bgra, unsigned char* mask,
                                 hipStream_t stream);
// block norm tiles (experiments/block_norm_visualization.py): run r of the table = the B = count fp32 maps [ih, iw] of one block, each normalised by
// its own min / max to uint8 and enlarged by the whole factors oh / ih, ow / iw into its tile of the packed out; minmax = [images of the table, 2]
int mdpt_launch_post_block_norm_tiles(const PostRunTable& t, unsigned char* out, float* minmax, hipStream_t stream);
// depth-to-mesh (the 3D viewer's "Save 3D Model": shaders.js run_vertex_shader_cpu, mesh.js _make_plane_mesh / filter_mesh_vertices): MeshJob above ->
// the kept vertices (xyz [B, nv, 3], uv [B, nv, 2]) and faces ([B, nf, 3] or, for points, [B, nv, 1]) packed at the front of each image's slab,
// counts [B, 2] = {kept vertices, kept faces}, bounds [B, 2, 3] = {min xyz, max xyz}. Five launches (four for points), no single-pass scan.
int mdpt_launch_post_mesh(const MeshJob& m, float* xyz, float* uv, unsigned* faces, int* counts, float* bounds, hipStream_t stream);
// rendering of depth meshes (the 3D viewer's render_3d): RenderJob above -> color uint8 BGRA [B, V, H, W, 4] (background 0, 0, 0, 0) and, where not
// null, depth fp32 [B, V, H, W] (clip-space w, background +inf) and ids int32 [B, V, H, W] (the face's index, background -1). Four launches.
int mdpt_launch_post_render(const RenderJob& r, unsigned char* color, float* depth, int* ids, hipStream_t stream);
// hole filling of rendered views (depth-banded push-pull): FillJob above. ceil(top / FILL_PUSH_LEVELS) push launches, one launch for the levels
// top .. L, top pull launches: the count follows from H and W alone. No atomics, bit-deterministic, the scratch's contents before do not matter.
int mdpt_launch_post_fill(const FillJob& j, hipStream_t stream);
// tiled high-resolution inference: tiles = T PostTile records on the device (maps of dtype dt). Fit: every tile's map against the guide (gh x gw,
// dtype gdt, covering the H x W photo) over the tile's box -> sums [T, 6] fp64 {n, Sx, Sy, Sxx, Sxy, Syy}, fit [T, 2] fp64 {scale, shift}; parts =
// [T, max_chunks, 6] fp64 scratch. Two launches, bit-deterministic. Blend: the feathered weighted mean of the fitted tiles -> out fp32 [H, W]; fit ==
// null: scale 1, shift 0; sums != null: a tile with n == 0 is skipped
int mdpt_launch_post_tile_fit(const PostTile* tiles, int T, int max_chunks, int dt, const void* guide, int gdt, int gh, int gw, int H, int W, double* parts,
                              double* sums, double* fit, hipStream_t stream);
int mdpt_launch_post_tile_blend(const PostTile* tiles, int T, int dt, int H, int W, const double* fit, const double* sums, double feather, float* out,
                                hipStream_t stream);

// true depth from ground truth: pairs = P AlignPair records on the device (predictions of dtype dt); inverse: t = 1 / truth and d = 1 / (A v + B),
// else t = truth and d = A v + B; a truth pixel counts inside [tmin, tmax]. Fit: sums [P, 6], fit [P, 2] fp64; least squares (median == 0) is two
// launches over parts, the median fit eleven (hist [P, ALIGN_HIST_WORDS], state [P, ALIGN_STATE_WORDS]). Metrics: [P, ALIGN_METRIC_SUMS] fp64, fit ==
// null: A = 1, B = 0. Apply: out fp32, pair p's H x W map at out + offs[p], clamped to [dmin, dmax] where finite; max_pixels = the largest H W (it
// sizes the grid). max_chunks = the chunks of the largest H x W. All bit-deterministic.
int mdpt_launch_post_align_fit(const AlignPair* pairs, int P, int max_chunks, int dt, int inverse, int median, double tmin, double tmax, double* parts,
                               unsigned* hist, unsigned* state, double* sums, double* fit, hipStream_t stream);
int mdpt_launch_post_align_metrics(const AlignPair* pairs, int P, int max_chunks, int dt, int inverse, double tmin, double tmax, const double* fit,
                                   double* parts, double* metrics, hipStream_t stream);
int mdpt_launch_post_align_apply(const AlignPair* pairs, int P, size_t max_pixels, int dt, int inverse, const double* fit, const long long* offs, double dmin,
                                 double dmax, float* out, hipStream_t stream);

// photo-guided upsampling (He & Sun's fast guided filter with the photo as guide): pairs = P GuidedPair records on the device (maps of dtype dt), each
// pair's scratch at scratch + scratch_off. Six launches whatever P is (cell sums, moment rows, moment columns + solve, coefficient rows, coefficient
// columns, apply); coeffs != null: pair p's mean coefficients fp64 [h, w, 4] also at coeffs + 4 sum_{q < p} h_q w_q. max_* = the largest of the table
// (they size the grids). Bit-deterministic.
int mdpt_launch_post_guided(const GuidedPair* pairs, int P, int dt, int radius, double eps, int max_h, int max_w, int max_H, int max_W, char* scratch,
                            double* coeffs, hipStream_t stream);

// temporally stable video depth (post_video.inc): frames = [T, hw] of dtype dt, prev = the raw last frame of the call before, started[0] != 0: there
// was one (else frame 0 starts the chain). Fit: table [T, 4] fp64 {A, B, sigma, cut}, ab_out [2] the last (A, B), sums (null: not wanted) [rounds + 1, T, 6];
// scratch = video_fit_scratch_doubles. 2 (rounds + 1) + 1 launches whatever T. Filter: one launch. Display: stable fp32 [T, h, w] -> BGR [T, oh, ow, 3]
// with the carried range (scaled null: no resize); four launches. All bit-deterministic, no atomics.
inline size_t video_fit_scratch_doubles(size_t T, size_t hw) { return T * tile_fit_chunks(hw) * 6 + T * 4; }
int mdpt_launch_post_video_fit(const void* frames, int dt, int T, size_t hw, const void* prev, const double* ab_in, const int* started, int rounds, double c,
                               double cut_corr, double* table, double* ab_out, double* sums, double* scratch, hipStream_t stream);
int mdpt_launch_post_video_filter(const void* frames, int dt, int T, size_t hw, const double* table, const float* prev_out, double alpha, double tau, float* out,
                                  hipStream_t stream);
int mdpt_launch_post_video_display(const float* stable, int T, int h, int w, int oh, int ow, const double* table, const float* range_in, const int* started,
                                   double rho, int reverse, const unsigned char* cmap, float* scaled, unsigned* parts, unsigned* rparts, unsigned char* u8,
                                   unsigned char* out, float* ranges, float* range_out, hipStream_t stream);

// synthetic depth of field (post_refocus.inc; a pair = mdpt_refocus_pair of include/mdpt.h): the h x w map (the table's dtype), the uint8 BGR photo of
// H x W pixels whose rows lie `pitch` bytes apart (any alignment), the packed uint8 H x W x 3 output (null in every record: the preparation alone),
// where the pair's scratch starts (bytes from the call's scratch pointer, a multiple of 8) and the number of 32 x 32 output tiles of the pairs before
// it. Device table, indexed by pair. A pair's scratch: REFOCUS_HEADER_BYTES ({min, max} partials of the map as ordered keys, then RefocusState),
// then 8 bytes per photo pixel: B | G << 8 | R << 16 | rq << 24 and the fp32 bits of the signed defocus.
struct RefocusPair { const void* map; int h, w; const unsigned char* photo; long long pitch; int H, W; unsigned char* out; long long scratch_off, tile_off; };
#define REFOCUS_MAX_RADIUS 32
#define REFOCUS_TILE 32    // output pixels of one gather workgroup along each axis (one thread each)
#define REFOCUS_PARTS 64   // workgroups that share the min / max of one map
#define REFOCUS_HEADER_BYTES 1024
inline size_t refocus_pair_scratch_bytes(size_t H, size_t W) { return REFOCUS_HEADER_BYTES + H * W * 8; }
inline size_t refocus_pair_tiles(size_t H, size_t W) { return ((H + REFOCUS_TILE - 1) / REFOCUS_TILE) * ((W + REFOCUS_TILE - 1) / REFOCUS_TILE); }
// one call: `focus` is the focal value (inverse space: 0 .. 1 of the map's own range; depth space: 1 / the focal depth) unless pointed, when it is read
// at the photo pixel under (fx, fy) on the device; half_range = focus_range / 2. radius_out / defocus_out (null: not wanted): every pair's rq and e32
// planes end to end in pair order. gather == 0: the preparation alone. Three launches and the gather whatever P is. Bit-deterministic, no atomics.
struct RefocusJob {
    const RefocusPair* pairs;
    int P, dt, depth_space, pointed, max_radius, gather;
    double focus, fx, fy, aperture, half_range;
    char* scratch;
    unsigned char* radius_out;
    float* defocus_out;
    size_t max_pixels, total_tiles;
};
int mdpt_launch_post_refocus(const RefocusJob& job, hipStream_t stream);

// surface normals and relighting (post_normals.inc; a pair = mdpt_normals_pair of include/mdpt.h): the h x w map (the table's dtype), the uint8 BGR photo
// of H x W pixels whose rows lie `pitch` bytes apart (null: every byte 255, a white-clay hillshade), the outputs (each null in every record or in none):
// fp32 [H,W,3] unit normals (x, y, z), uint8 [H,W,3] encoded normals (B, G, R = z, y, x) and uint8 [V,H,W,3] relit frames, where the pair's scratch
// starts (NORMALS_HEADER_BYTES: the {min, max} partials of the map as ordered keys, then NormalsState), the 32 x 32 output tiles of the pairs before it,
// the camera's kx = x_scale tan(fov / 2), ky = y_scale tan(fov / 2) and the difference step in photo pixels. Device table, indexed by pair.
struct NormalsPair {
    const void* map; int h, w; const unsigned char* photo; long long pitch; int H, W; float* normals; unsigned char* encoded; unsigned char* relit;
    long long scratch_off, tile_off; double kx, ky; int step, pad;
};
#define NORMALS_MAX_STEP 16
#define NORMALS_TILE 32      // output pixels of one workgroup along each axis (one thread each)
#define NORMALS_MAX_LIGHTS 64
#define NORMALS_PARTS 64     // workgroups that share the min / max of one map
#define NORMALS_HEADER_BYTES 1024
inline size_t normals_pair_tiles(size_t H, size_t W) { return ((H + NORMALS_TILE - 1) / NORMALS_TILE) * ((W + NORMALS_TILE - 1) / NORMALS_TILE); }
// one call: z = 1 / (depth_a + depth_b v) with v = the map in its own range (inverse space), or z = the map (depth space: no min / max launches).
// lights: V unit directions, fp64 [V,3], device memory (null: no frames). central_only: edge_ratio = inf. At most three launches whatever P and V.
struct NormalsJob {
    const NormalsPair* pairs;
    int P, dt, depth_space, central_only, V, shininess_log2;
    double depth_a, depth_b, edge_ratio, ambient, diffuse, specular;
    const double* lights;
    char* scratch;
    size_t total_tiles;
};
int mdpt_launch_post_normals(const NormalsJob& job, hipStream_t stream);

// cast shadows and ambient occlusion for the relighting (post_shadows.inc; a pair = mdpt_shadows_pair of include/mdpt.h): a NormalsPair's map, photo, relit
// frames, scratch header, photo tiles, camera and step, and the pair's working grid of gh x gw nodes with its planes - ao fp32 [gh,gw] and vis fp32
// [V,gh,gw], each null in every record or in none - and gtile_off, the 32 x 32 grid tiles of the pairs before it. Device table, indexed by pair.
struct ShadowsPair {
    const void* map; int h, w; const unsigned char* photo; long long pitch; int H, W, gh, gw; float* ao; float* vis; unsigned char* relit;
    long long scratch_off, tile_off, gtile_off; double kx, ky; int step, pad;
};
#define SHADOWS_MAX_REACH 32     // grid nodes a shadow march or an occlusion direction walks at most: the halo of the grid kernel's LDS image
#define SHADOWS_AO_DIRECTIONS 8
// one call: the fields of a NormalsJob under their names (the shade kernel is normals_tile_kernel's body), the marches' controls and which planes the
// shade kernel reads (use_vis: shadow_reach > 0; use_ao: ao_reach > 0 and ao_strength > 0; else the factor is the constant 1). At most four launches.
struct ShadowsJob {
    const ShadowsPair* pairs;
    int P, dt, depth_space, central_only, V, shininess_log2;
    double depth_a, depth_b, edge_ratio, ambient, diffuse, specular;
    const double* lights;
    char* scratch;
    size_t total_tiles, total_gtiles;
    int shadow_reach, ao_reach, thick_inf, use_vis, use_ao, planes, shade, pad;
    double shadow_bias, shadow_thickness, ao_radius, ao_bias, ao_strength;
};
int mdpt_launch_post_shadows(const ShadowsJob& job, hipStream_t stream);

// depth segmentation (post_segment.inc; an image = mdpt_segment_image of include/mdpt.h): the h x w map (the table's dtype), its int32 [h,w] label plane
// (the parents of the union-find until the relabel launch), where the image's scratch starts, the rows of the region tables, the 32 x 32 tiles and the
// nodes of the images before it. Device table, indexed by image. An image's scratch: SEGMENT_HEADER_BYTES ({min, max} partials of the map as ordered
// keys, then SegmentState), an int32 plane (a root's area, then its new id), a byte plane of link bits, the kept roots of every 256-node block.
struct SegmentImage { const void* map; int h, w; int* labels; long long scratch_off, region_off, tile_off, pixel_off; };
#define SEGMENT_TILE 32      // nodes of one union-find workgroup along each axis (one thread each)
#define SEGMENT_PARTS 64     // workgroups that share the min / max of one map
#define SEGMENT_HEADER_BYTES 1024
inline size_t segment_image_tiles(size_t h, size_t w) { return ((h + SEGMENT_TILE - 1) / SEGMENT_TILE) * ((w + SEGMENT_TILE - 1) / SEGMENT_TILE); }
inline size_t segment_image_scratch_bytes(size_t h, size_t w) {
    const size_t n = h * w;
    return (SEGMENT_HEADER_BYTES + 4 * n + ((n + 7) & ~(size_t)7) + (n + 255) / 256 * 4 + 7) & ~(size_t)7;
}
inline size_t segment_image_regions(size_t h, size_t w, size_t min_area) { return (h * w) / min_area; }  // (min_area >= 1: at most h w)
// one call: the region tables (rows region_off .. of image i) - area int32, bbox int32 x 4 {x0, y0, x1, y1}, first int32, vrange fp32 x 2 {vmin, vmax},
// sum_q int64 - counts int32 [P] and range fp64 [P, 2] = {lo, hi}. Ten launches whatever P is. Integer atomics only, bit-deterministic.
struct SegmentJob {
    const SegmentImage* images;
    int P, dt, depth_space, conn8, min_area, pad;
    double step;
    char* scratch;
    int* counts; int* area; int* bbox; int* first; float* vrange; long long* sum_q; double* range;
    size_t max_pixels, max_regions, total_tiles;
};
int mdpt_launch_segment(const SegmentJob& job, hipStream_t stream);
// label -> BGR through a fixed integer hash (-1: black): colors = uint8 [nodes of the call, 3] in image order
int mdpt_launch_segment_colors(const SegmentImage* images, int P, size_t max_pixels, unsigned char* colors, hipStream_t stream);
// pick-to-cutout (a photo = mdpt_segment_photo of include/mdpt.h): the int32 [h,w] labels, the uint8 BGR photo of H x W pixels whose rows lie `pitch`
// bytes apart, its BGRA [H,W,4] and mask [H,W] outputs, where the image's rows of `selected` start and how many it has. picks = int32 [num_picks, 2]
// {image, node (by_label == 0) or region (by_label != 0)} on the device; selected = uint8, one per region row, zero on entry. Two launches.
struct SegmentPhoto { const int* labels; int h, w; const unsigned char* photo; long long pitch; int H, W; unsigned char* bgra; unsigned char* mask; long long region_off; int regions, pad; };
int mdpt_launch_segment_cutout(const SegmentPhoto* photos, int P, const int* picks, int num_picks, int by_label, unsigned char* selected, int invert,
                               size_t max_groups, hipStream_t stream);

// locally varying true-depth alignment (post_localfit.inc; a pair = mdpt_localfit_pair of include/mdpt.h): an AlignPair (the same seven fields first, so
// that the sample rule of post_align.inc reads it), the gh x gw grid, the cells of the pairs before it (rows of the moment and coefficient tables),
// where the pair's scratch starts and, for the apply launch, its fp32 H x W output. Device table, indexed by pair. A pair's scratch: the partial
// moments [cells][chunks of its largest cell][6], then the window fits [cells][2], fp64.
struct LocalFitPair { const void* pred; int ph, pw; const float* truth; const unsigned char* valid; int H, W, gh, gw; long long cell_off, scratch_off; float* out; };
#define LOCALFIT_MAX_GRID 256   // cells along an axis, at most
#define LOCALFIT_MAX_RADIUS 64  // window radius in cells, at most
// the chunks (MDPT_TILE_FIT_CHUNK pixels, row-major inside the cell) of the largest cell: a cell spans at most ceil(H / gh) x ceil(W / gw) pixels
__host__ __device__ inline size_t localfit_cell_chunks(size_t H, size_t W, size_t gh, size_t gw) { return tile_fit_chunks(((H + gh - 1) / gh) * ((W + gw - 1) / gw)); }
inline size_t localfit_pair_scratch_bytes(size_t H, size_t W, size_t gh, size_t gw) {
    return (gh * gw * localfit_cell_chunks(H, W, gh, gw) * 6 + gh * gw * 2) * sizeof(double);
}
// fit: five launches whatever P is (cell partials, cells, global fit, window fits, coefficient means) -> moments [cells of the call, 6], fit [P, 2],
// sums [P, 6], coeffs [cells of the call, 2]; max_blocks / max_cells: the largest cells x chunks / cells of a pair. apply: one launch.
struct LocalFitJob {
    const LocalFitPair* pairs;
    int P, dt, inverse, radius;
    double prior, tmin, tmax;
    char* scratch;
    double* moments; double* fit; double* sums; double* coeffs;
    size_t max_blocks, max_cells;
};
int mdpt_launch_localfit_fit(const LocalFitJob& job, hipStream_t stream);
int mdpt_launch_localfit_apply(const LocalFitPair* pairs, int P, size_t max_pixels, int dt, int inverse, const double* coeffs, double dmin, double dmax,
                               hipStream_t stream);

// stream_probe.hip: does `candidate` run kernels beside `waiter_stream`? (*seen != 0 after synchronising with waiter_stream)
int mdpt_launch_queue_probe(unsigned* flag, unsigned* seen, hipStream_t waiter_stream, hipStream_t candidate, hipEvent_t ready);

// ------------------------------------------------------------------------------------------------
// launchers: one set per operand format (op_types.h). A kernel file sees its own set through MDPT_FN; the host side (mdpt_internal.h)
// includes mdpt_launchers.inc a second time for the other format and picks per handle (OPL). C linkage: the two
// builds of a file differ in what `op_t*` points at, which must not reach the symbol names.
// ------------------------------------------------------------------------------------------------
extern "C" {
#include "mdpt_launchers.inc"
}
