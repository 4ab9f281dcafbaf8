// Launcher declarations of the operand-format dependent kernel files; included by mdpt_kernels.h with MDPT_FN(name) = name##_bf16 or
// name##_f16 (no include guard on purpose: mdpt_internal.h includes it once per operand format).
int MDPT_FN(mdpt_launch_gemm)(const GemmParams& p, hipStream_t stream);   // returns hipError_t as int
bool MDPT_FN(mdpt_gemm_resolves_to_pp256)(const GemmParams& p);          // would mdpt_launch_gemm run the 8-phase 256x256 kernel for p?
bool MDPT_FN(mdpt_conv3h_supported)(const Conv3hParams& p);
int MDPT_FN(mdpt_launch_conv3h)(const Conv3hParams& p, hipStream_t stream);
int MDPT_FN(mdpt_launch_attention)(const AttnParams& p, hipStream_t stream);
// diagnostic: explicit softmax(q k^T + bias [+ shift mask]) as fp32 [B, heads, N, N] from the same Q / K planes (head dim 64 families;
// SwinV2 windows: B = images * windows, head dim 32)
int MDPT_FN(mdpt_launch_attn_weights)(const AttnParams& p, float* out_bhnn, hipStream_t stream);
// ---- ew_norm.inc
// LayerNorm over the last dim (eps 1e-6): fp32 rows -> bf16 hi (+lo) (+ optional fp32 copy)
// out_f8 / out_a8 (here and below): the lo plane in the fp8 form an F8 consumer reads (GemmParams::out_f8, f8_cross.h)
int MDPT_FN(mdpt_launch_layernorm)(const float* x, const float* gamma, const float* beta, op_t* out_hi, op_t* out_lo,
                          float* out_f32, int rows, int F, hipStream_t stream, size_t out_f8 = 0, int out_a8 = 0);
// the same on x + part[0] + ... + part[npart-1] (fp32 [rows, F] each, part_stride elements apart: the partial sums of a K-split GEMM), x updated
int MDPT_FN(mdpt_launch_layernorm_addp)(float* x, const float* part, size_t part_stride, int npart, const float* gamma, const float* beta,
                                       op_t* out_hi, op_t* out_lo, float* out_f32, int rows, int F, hipStream_t stream, size_t out_f8 = 0, int out_a8 = 0);
// finishing kernel of a K split whose ranges all stored partial planes (GemmParams::ks_all): sum in the order z = 0, 1, ... (+ bias) -> fp32 rows / planes
int MDPT_FN(mdpt_launch_ksplit_finish)(const float* part, size_t part_stride, int nparts, const float* bias, float* out_f32, op_t* out_hi, op_t* out_lo,
                                      int relu_planes, int M, int N, int ldc, hipStream_t stream, size_t out_f8 = 0, int out_a8 = 0);
// per-token L2 norm of fp32 rows [B, npad, F]: rows skip .. skip + ntok - 1 of every image -> norm_out [B, ntok] and / or channel `chan` of
// the same rows -> chan_out [B, ntok] (either may be null); one wave per row, no atomics, batch-invariant summation order
int MDPT_FN(mdpt_launch_row_norm)(const float* in, float* norm_out, float* chan_out, int chan, int B, int ntok, int npad, int skip, int F,
                                  hipStream_t stream);
// ViT-G SwiGLU gate: fp32 [rows, 2h] -> silu(first half) * second half as bf16 hi (+lo) [rows, hp] (pad columns zero)
int MDPT_FN(mdpt_launch_swiglu)(const float* in, op_t* out_hi, op_t* out_lo, size_t rows, int h, int hp, hipStream_t stream);
// token-mean compensation of the weight rounding (fp16 modes): per-image column means of an operand plane over every step-th real row,
// written as the [B, K] A operand of the small GEMM against the weight residue (lo) plane
int MDPT_FN(mdpt_launch_colmean)(const op_t* A, int lda, int B, int rows_per_img, int nreal, int step, int K, op_t* mean, hipStream_t stream);
// ... and that product itself: out[b][n] = bias[n] + sum_k mean[b][k] * w_lo[n][k] (fp32 table, row stride N; K % 32 == 0)
int MDPT_FN(mdpt_launch_wrc_table)(const op_t* mean, const op_t* w_lo, const float* bias, float* out, int B, int N, int K, hipStream_t stream, const float* wscale = nullptr);
// ---- ew_tokens.inc
// NCHW image (fp32 / bf16 / fp16: img_dtype) -> im2col rows [B*Np, Kp] bf16 hi (+lo), k = c*P*P + ky*P + kx, zero padded to Kp
// poison != null: word b is set when image b holds a NaN / inf (mdpt_forward's non-finite propagation)
int MDPT_FN(mdpt_launch_patchify)(const void* img, int img_dtype, op_t* out_hi, op_t* out_lo, int B, int H, int W, int P, int Kp,
                         hipStream_t stream, unsigned* poison = nullptr);
// depth [B, hw] (depth_dtype): the maps of the images whose poison word is set become NaN
int MDPT_FN(mdpt_launch_poison_depth)(void* depth, int depth_dtype, const unsigned* poison, int B, size_t hw, hipStream_t stream);
// bicubic (A=-0.75, align_corners=False) resize of the [Gh*Gw, F] position grid to [gh*gw, F]
int MDPT_FN(mdpt_launch_posembed)(const float* base, float* out, int Gh, int Gw, int gh, int gw, int F, hipStream_t stream);
// residual-stream init: cls rows = cls_token + cls_embedding, pad rows = 0 (patch rows are written by E_PATCH)
int MDPT_FN(mdpt_launch_init_tokens)(float* resid, const float* cls_token, const float* cls_embed, int B, int N, int npad, int F,
                            hipStream_t stream);
// zero the pad columns [N, npadv) of the transposed-V planes
int MDPT_FN(mdpt_launch_zero_vt_pad)(op_t* vt_hi, op_t* vt_lo, int rows, int N, int npadv, hipStream_t stream);
int MDPT_FN(mdpt_launch_tokens_import)(const float* in, op_t* out_hi, op_t* out_lo, int B, int N, int npad, int F,
                              hipStream_t stream, size_t out_f8 = 0, int out_a8 = 0);
int MDPT_FN(mdpt_launch_tokens_export)(const op_t* in_hi, const op_t* in_lo, const float* in_f32, float* out, int B, int N,
                              int npad, int F, int skip_cls, hipStream_t stream, size_t lo_f8 = 0);  // lo_f8: in_lo is an e5m2 residue plane (Planes::f8)
// stage-level encoder entry: resid[b, 1+t, :] = tokens[b, t, :] + pos[t, :]
int MDPT_FN(mdpt_launch_tokens_to_resid)(const float* tokens, const float* pos, float* resid, int B, int Np, int npad, int F,
                                hipStream_t stream);
// BEiT relative position bias (reference v31_beit/components/relative_positional_encoder.py:117-309): bilinear-resize the
// learned [(2Gh-1)(2Gw-1)+3, heads] table to the current grid and lay it out per head as an extended LUT so that the bias of
// (query q, key k) is ext[tq[q] - tk[k]] including the three cls cases; also fills the per-token index terms tq / tk.
int MDPT_FN(mdpt_launch_beit_relpos)(const float* ref_lut, float* ext_lut, int* tq, int* tk, int heads, int Gh, int Gw, int gh, int gw,
                            int N, int ntok_pad, hipStream_t stream);
int MDPT_FN(mdpt_beit_relpos_elen)(int gh, int gw);
int MDPT_FN(mdpt_launch_beit_relpos_batch)(const BeitRelposBatch& b, hipStream_t stream);
// ---- ew_resize.inc
// bilinear align_corners=True resize of fp32 NHWC [B,Hi,Wi,C] -> [B,Ho,Wo,C] as bf16 hi (+lo) and/or fp32
int MDPT_FN(mdpt_launch_upsample)(const float* in, op_t* out_hi, op_t* out_lo, float* out_f32, int B, int Hi, int Wi, int Ho,
                         int Wo, int C, hipStream_t stream, size_t out_f8 = 0, int out_a8 = 0);
// the same resize of a bf16 NHWC map to a bf16 NHWC map (C % 8 == 0), arithmetic of up_bf16.h
int MDPT_FN(mdpt_launch_upsample_bf16)(const op_t* in, op_t* out, int B, int Hi, int Wi, int Ho, int Wo, int C, hipStream_t stream);
// ---- ew_pack.inc
// row_scale != null (MDPT_PACK_LINEAR only): row n is multiplied by row_scale[n] in fp32 BEFORE the bf16 split (a per-output-feature
// layer scale folded into the weights: diag(gamma) W)
int MDPT_FN(mdpt_launch_pack_weight)(const void* src, int src_dtype, op_t* dst_hi, op_t* dst_lo, int kind, int N, int K, int Np, int Kp,
                            int ksz, hipStream_t stream, int src_ld = 0, int src_col0 = 0, const void* row_scale = nullptr, int scale_dtype = 0,
                            const float* wscale = nullptr);  // wscale: device {s, 1 / s}, every entry is multiplied by s (a power of two) before the split
// fp8 planes of an F8 class (fp16 build; f8_cross.h): w8 / wlo8 [Np][Kp] e4m3 bytes of W_hi / W - W_hi in the fp8 K order (conv: 128-channel blocks),
// scales [2 Np] E8M0 bytes (row scales of w8, then of wlo8 with the activations' 2^F8_LO_SHIFT folded in); Kp % 128 == 0; wlo8 may be null (two terms)
int MDPT_FN(mdpt_launch_pack_weight_f8)(const void* src, int src_dtype, unsigned char* w8, unsigned char* wlo8, unsigned char* scales, int kind, int N, int K,
                                       int Np, int Kp, int ksz, hipStream_t stream, int src_ld = 0, int src_col0 = 0, const void* row_scale = nullptr,
                                       int scale_dtype = 0, const float* wscale = nullptr);
// scale2 = {s, 1 / s}: the power of two that puts the largest |row_scale[n] * src[n][k]| of the matrix in [2^13, 2^14) (fp16 build: keeps the lo
// plane of a layer-scale-folded matrix out of the subnormal range; GemmParams::wscale undoes it exactly)
int MDPT_FN(mdpt_launch_weight_scale)(const void* src, int src_dtype, int N, int K, int src_ld, int src_col0, const void* row_scale, int scale_dtype, float* scale2,
                                     hipStream_t stream, int always = 0);  // always: scale whatever the largest entry is (mdpt_debug_set_wscale_policy)
// fp32 vector copy with zero padding (biases); `rep` repeats are not needed: plain copy
int MDPT_FN(mdpt_launch_pad_copy_f32)(const void* src, int src_dtype, float* dst, int n, int np, hipStream_t stream, const void* scale = nullptr,
                             int scale_dtype = 0, float mul = 1.0f);  // dst = float(src) (* float(scale)) (* mul)
int MDPT_FN(mdpt_launch_memset_f32)(float* dst, float value, size_t n, hipStream_t stream);
int MDPT_FN(mdpt_launch_add_f32)(float* dst, const float* src, size_t n, hipStream_t stream);  // dst += src
// ---- ew_layout.inc: layout conversions for the stage-level API / debug taps
int MDPT_FN(mdpt_launch_nhwc_to_nchw)(const float* in_f32, const op_t* in_hi, const op_t* in_lo, float* out, int B, int H, int W,
                             int C, int Cp, hipStream_t stream);
int MDPT_FN(mdpt_launch_nchw_to_nhwc)(const float* in, float* out_f32, op_t* out_hi, op_t* out_lo, int relu_bf16, int B, int H,
                             int W, int C, int Cp, hipStream_t stream, size_t out_f8 = 0, int out_a8 = 0);
// ---- ew_prepare.inc
// uint8 HWC BGR -> normalised fp32 [3,oh,ow] RGB through PyTorch-compatible antialiased bilinear resize; bgr = the first pixel of an ih x iw box of an
// image whose rows are `pitch` bytes apart (3 iw: a packed image)
int MDPT_FN(mdpt_launch_prepare_image)(const unsigned char* bgr, size_t pitch, void* out, int out_dtype, int ih, int iw, int oh, int ow, const float mean[3],
                              const float inv_std[3], int interp, hipStream_t stream);
// ... fused with patchify for the frames of a BgrRunTable (at most 65535), written from im2col row 0 of out_hi / out_lo
int MDPT_FN(mdpt_launch_prepare_patchify)(const BgrRunTable& t, int img_dtype, op_t* out_hi, op_t* out_lo, int H, int W, int P, int Kp,
                                         const float mean[3], const float inv_std[3], int interp, hipStream_t stream);  // interp: 0 bilinear, 1 bicubic (both antialiased)
// ---- head.hip
bool MDPT_FN(mdpt_head_tail_supported)(int cin);
bool MDPT_FN(mdpt_head_tail_scale_ok)(int Hi, int Wi, int Ho, int Wo);
int MDPT_FN(mdpt_launch_head_tail)(const HeadTailParams& p, int cin, hipStream_t stream);
// ---- swin.hip
// out = LN_eps(x [+ part]) (+ add): fp32 rows -> fp32 (may alias add) and/or bf16 hi (+lo); part = partial sums of a K-split GEMM's second range
int MDPT_FN(mdpt_launch_ln_res)(const float* x, const float* add, const float* gamma, const float* beta, float eps, float* out_f32,
                       op_t* out_hi, op_t* out_lo, int rows, int F, hipStream_t stream, int ld_planes = 0, const float* part = nullptr);
// window -> image token map (with cyclic shift sh, sw), shifted-window region ids [nW][region_ld], window-local tq / tk terms
// tokmap / vtokmap (optional): the inverse, image token -> w * tok_stride + i resp. w * vtok_stride + i
int MDPT_FN(mdpt_launch_swin_window_map)(int* rowmap, int* region, int* tq, int* tk, int gh, int gw, int wh, int ww, int sh, int sw,
                                int region_ld, int ntok_pad, hipStream_t stream, int* tokmap = nullptr, int tok_stride = 0, int* vtokmap = nullptr,
                                int vtok_stride = 0);
// continuous position bias LUT [heads][(2wh-1)(2ww-1)] = 16*sigmoid(MLP(log-coords)); pretrained = 0 means "None"
int MDPT_FN(mdpt_launch_swin_cpb)(const float* w1, const float* b1, const float* w2, float* lut, int heads, int hidden, int wh, int ww,
                         int pretrained, hipStream_t stream);
int MDPT_FN(mdpt_launch_swin_cpb_batch)(const SwinCpbBatch& b, hipStream_t stream);
// fp32 qkv [B*N, 3F] -> normalised/scaled window operands Q,K [B*nw, heads, npad, 32] and Vt [B*nw, heads, 32, npadv]
int MDPT_FN(mdpt_launch_swin_qkv_prep)(const float* qkv, const int* rowmap, const float* logit_scale, op_t* q_hi, op_t* q_lo,
                              op_t* k_hi, op_t* k_lo, op_t* vt_hi, op_t* vt_lo, int B, int N, int nw, int wa, int npad,
                              int npadv, int heads, hipStream_t stream, bool qk = true);  // qk = false: V only (Q, K came out of the GEMM)
// fp32 [B,gh,gw,C] -> bf16 rows [B*(gh/2)*(gw/2), 4C] = cat(TL, BL, TR, BR)
int MDPT_FN(mdpt_launch_swin_merge_gather)(const float* tok, op_t* out_hi, op_t* out_lo, int B, int gh, int gw, int C,
                                  hipStream_t stream);
int MDPT_FN(mdpt_launch_f32_to_planes)(const float* in, op_t* out_hi, op_t* out_lo, size_t rows, int F, int ld, hipStream_t stream);
