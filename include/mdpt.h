/* libmdpt - C ABI of the MI355X-native DPT depth-inference path (Depth-Anything-V2 family).
 *
 * The reference (heyoeyo/muggled_dpt) has NO FFI / operator / plugin layer: its boundary is the Python API
 *   make_dpt_from_state_dict()            muggled_dpt/make_dpt.py:21-72
 *   DPTModel.forward / .inference         muggled_dpt/dpt_model.py:61-83, :87-109
 *   model.patch_embed / .imgencoder / .reassemble / .fusion / .head   (dpt_model.py:50-54; called one by one in
 *                                          simple_examples/internal_features.py:38-45)
 * This header is therefore the NEW boundary a binding of that API sits on: plain pointers and
 * sizes, no torch types. Every entry point names the reference call it replaces.
 *
 * Conventions
 *   - return value: 0 = OK, otherwise a negative MDPT_E_* code or a positive hipError_t; mdpt_last_error() has text.
 *   - all `dev` pointers are device (HBM) pointers owned by the caller (PyTorch allocates them in our binding);
 *     the library allocates no device memory and does not synchronise with the host (one exception: the probe below).
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream). Every kernel is ordered on the caller's stream. ONE
 *     exception, stated here because it is visible to tools: mdpt_forward lazily creates an internal non-blocking side stream + two events
 *     per handle. The first forward on a caller stream picks that side stream among up to four candidates by PROBING, on the GPU, that it
 *     runs beside the caller's stream and not behind it on a shared hardware queue (a few tiny launches and one host wait, once per handle
 *     and caller stream, skipped inside a stream capture; mdpt_debug_set_side_stream_probe). For batches >= 8 (mdpt_set_batch_split) the
 *     second half batch runs there; for smaller batches of the wide encoders (feature width >= 1024, default mode) the four reassembly
 *     branches do, each as soon as its encoder tap exists (mdpt_debug_set_reassemble_overlap). Either way the side stream is
 *     forked from and joined back into the caller's stream with events before the call returns (also on the error path) - stream-ordering
 *     semantics for the caller are unchanged, the call stays capturable into a hipGraph, results are bit-identical to the one-stream form.
 *   - tensors at this boundary use the REFERENCE layouts: images/maps BCHW, tokens B x N x F, depth B x H x W. The hot entry points
 *     (mdpt_bind_weight, mdpt_forward, mdpt_allgather) take a dtype tag per tensor (fp32, bf16 or fp16: whatever the caller's
 *     model dtype is - no cast kernels at the boundary); the stage-level / debug entry points are fp32.
 *   - a handle is not thread-safe; distinct handles are independent.
 */
#ifndef MDPT_H
#define MDPT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDPT_ABI_VERSION 6

/* arithmetic modes (all accumulate in fp32; residual stream, LayerNorm and softmax statistics are fp32) */
#define MDPT_PREC_BF16 0   /* bf16 MFMA operands - the reference's GPU default dtype (demo_helpers/misc.py:73-77) */
#define MDPT_PREC_BF16X3 1 /* split-bf16 (hi+lo) operands, 3 MFMA passes: fp32-class accuracy (parity mode)        */
#define MDPT_PREC_FP16 2   /* fp16 MFMA operands (v_mfma_*_f16: the bf16 rate, 11 instead of 8 significand bits; converts saturate at
                              +-65504 - and turn a NaN into a finite value; a NaN / inf in the input IMAGE still gives a NaN depth map,
                              in every mode: mdpt_set_nonfinite_propagation) - what the reference's device policy hands the model when
                              bf16 is not preferred (demo_helpers/misc.py:61-77: float16). The layer-scale-folded matrices are packed
                              times a power of two that the GEMMs undo exactly, so checkpoints with gammas of 1e-2 ... 1e-5 keep their
                              hi / lo planes in fp16's normal range                                                   */
#define MDPT_PREC_FP16X3 3 /* split-fp16 (hi+lo) operands, 3 passes. Range: fp32-class while the largest |value| M of every operand
                              tensor lies in [2^-2, 32768]. Below, the lo plane (|A_lo| <= 2^-12 |A|) turns fp16-subnormal for the
                              typical element - an absolute 2^-25 floor; measured on the decoder stages: the max-norm error is
                              <= 1.25x its value at M ~ 4 down to M = 2^-2, 1.6 ... 2.8x at 2^-4, ~100x at 2^-10. Above 32768 the
                              hi planes approach saturation (65504). (tests/test_gpu_operand_range.py)                */
#define MDPT_PREC_MIXED 4  /* fp16 operands; the op classes listed in mdpt_default_mixed_passes() run 3 or 2 passes, the others 1:
                              the cheapest per-class assignment that keeps the depth map within 1e-3 of the fp32 reference
                              (profiles/r05_precision_budget.md). Range of the decoder classes (fp8 cross terms, MDPT_PASSES_2F8 /
                              _3F8 below): largest |activation| of an operand tensor in [2^-5, 32768]                         */

/* op classes of the path (what mdpt_set_class_passes / MDPT_PREC_MIXED address) */
#define MDPT_CLASS_PATCH 0  /* patch-embed projection                    patch_embed.py:92                         */
#define MDPT_CLASS_QKV 1    /* attention QKV projection                  transformer_block.py:160                  */
#define MDPT_CLASS_ATTN 2   /* q k^T and p v inside the attention kernel transformer_block.py:164                  */
#define MDPT_CLASS_PROJ 3   /* attention output projection (+ SwinV2 patch merge)   transformer_block.py:168       */
#define MDPT_CLASS_FC1 4    /* MLP first linear                          misc_helpers.py:111                       */
#define MDPT_CLASS_FC2 5    /* MLP second linear                         misc_helpers.py:115                       */
#define MDPT_CLASS_REASM 6  /* reassembly convs (incl. BEiT readout)     reassembly_model.py:139-149               */
#define MDPT_CLASS_FUSION 7 /* RefineNet fusion: the 3x3 convs of the projection path's residual conv unit  fusion_model.py:151-154,210-220 */
#define MDPT_CLASS_HEAD 8   /* depth head, first 3x3 conv (C -> C/2)     head_model.py:74-76                       */
#define MDPT_CLASS_FUSION_IN 9 /* the fusion blocks' conv_reassembly units (RCU on the reassembly map before the prior is added),
                                  fusion_model.py:148-150: the least error-sensitive convs of the decoder                  */
#define MDPT_CLASS_HEAD_TAIL 10   /* depth head behind its upsample: 3x3 conv C/2 -> 32 (the 32 -> 1 projection runs in fp32)  head_model.py:78-85 */
#define MDPT_CLASS_FUSION_PROJ 11 /* the 1x1 output projection of every fusion block                                            fusion_model.py:178-182 */
#define MDPT_NUM_CLASSES 12

#define MDPT_FAMILY_DAV2 0
#define MDPT_FAMILY_DAV1 1
#define MDPT_FAMILY_BEIT 2
#define MDPT_FAMILY_SWINV2 3

#define MDPT_E_INVALID (-1)    /* bad argument / shape                                  */
#define MDPT_E_STATE (-2)      /* call order (e.g. forward before finalize)             */
#define MDPT_E_MISSING (-3)    /* a weight required by the config was not bound         */
#define MDPT_E_SHAPE (-4)      /* bound weight has the wrong shape                      */
#define MDPT_E_WORKSPACE (-5)  /* workspace / packed buffer too small                   */
#define MDPT_E_UNSUPPORTED (-6)/* config outside this build (e.g. head dim != 64)        */
#define MDPT_E_GRID (-7)       /* odd patch grid: the reference raises RuntimeError at fusion_model.py:151 */

typedef struct mdpt_handle mdpt_handle;

/* == the 11-key config dict of the reference (state_dict_conversion/config_from_original_state_dict.py:29-41),
 *    minus the two Python-only flags, plus the arithmetic mode. */
typedef struct mdpt_config {
    int32_t features_per_token;
    int32_t num_heads;
    int32_t num_blocks;
    int32_t reassembly_features[4];
    int32_t base_patch_grid_h, base_patch_grid_w;
    int32_t fusion_channels;
    int32_t patch_size_px;
    int32_t is_giant;  /* ViT-G: SwiGLU FFN instead of the GELU MLP (components/misc_helpers.py:125-185); Depth-Anything V2 only */
    int32_t is_metric; /* sigmoid instead of the final ReLU (head_model.py:84) */
    int32_t precision; /* MDPT_PREC_* */
    int32_t family;    /* MDPT_FAMILY_DAV2: Depth-Anything V2 (encoder tapped after each quarter of the blocks, image_encoder_model.py:88-93)
                          MDPT_FAMILY_DAV1: Depth-Anything V1 (tapped after each of the last four blocks,
                                            v1_depthanything/image_encoder_model.py:55-61; parameters named imgencoder.blocks.N...)
                          MDPT_FAMILY_BEIT: MiDaS v3.1 BEiT (v31_beit/: relative-position-bias attention with q/v bias, no position
                                            embedding or out-norm, readout projection in the reassembly, patch 16)
                          MDPT_FAMILY_SWINV2: MiDaS v3.1 SwinV2 (v31_swinv2/: 4 stages of shifted-window cosine attention, head dim 32,
                                            post-norm blocks, patch merging between stages, patch 4). Uses the swin_* fields below;
                                            features per stage = reassembly_features[], features_per_token = reassembly_features[0] */
    /* SwinV2 only (make_swinv2_dpt.py:67-79); ignored by the other families */
    int32_t swin_heads[4];             /* heads_per_stage */
    int32_t swin_layers[4];            /* layers_per_stage (even: blocks come in plain/shifted pairs, image_encoder_model.py:155-161) */
    int32_t swin_window_h, swin_window_w;
    int32_t swin_pretrained_window[4]; /* pretrained_window_sizes_per_stage, 0 = None */
} mdpt_config;

int mdpt_abi_version(void);
const char* mdpt_last_error(void);

/* replaces make_depthanythingv2_dpt(**config) (make_depthanythingv2_dpt.py:67-138): validates the config and
 * derives the list of parameters the model needs. */
int mdpt_create(const mdpt_config* cfg, mdpt_handle** out);
void mdpt_destroy(mdpt_handle* h);

/* Per-class MFMA pass count on top of whatever mdpt_config.precision chose: 1 = one rounded 16-bit plane per operand; 3 = hi + lo planes
 * for both operands (A_lo W_hi + A_hi W_lo + A_hi W_hi, fp32-class); 2 = ACTIVATIONS split, weights one plane (A_lo W_hi + A_hi W_hi) -
 * for the decoder classes whose error is the rounding of their activations, two thirds of the cost of 3 (not for MDPT_CLASS_ATTN, whose
 * operands are both activations).
 * MDPT_PASSES_2F8 / MDPT_PASSES_3F8 (fp16 operand modes; MDPT_CLASS_REASM, _FUSION, _FUSION_IN, _FUSION_PROJ, _HEAD): the same two / three
 * products with the CROSS TERMS (A_lo W_hi, A_hi W_lo: 2^-11 of the main term) on fp8 operands through gfx950's block-scaled MFMA at twice
 * the fp16 rate - activations E5M2 with one constant power-of-two scale, weights E4M3 with one power-of-two scale per output row
 * (csrc/f8_cross.h) - i.e. 1.5 / 2 pass-equivalents instead of 2 / 3 at the accuracy of the fp16 cross terms
 * (tests/precision_budget/emulate_operand_rounding.py, format "sf8"). Range: the largest |activation| M of an operand tensor in
 * [2^-5, 32768] - the residue plane is e5m2(A_lo * 2^11), unsaturated for every normal fp16 value (<= 32768 < 57344), normal from a residue of
 * 2^-25 up; the a8 plane e5m2(A_hi) saturates at 57344. tests/test_gpu_operand_range.py sweeps M over this range: the error of the fp8 forms
 * stays within 1.3x its value at M ~ 4 and they keep carrying what the fp16 cross terms carry (the reassembly / fusion forms alone hold down
 * to M = 2^-9; a 3-term head in front of a head tail on fp16 planes sees that tail's floor from 2^-6). A class whose contraction lengths
 * are not all multiples of 128 (the small encoders' reassembly widths, fusion widths below 128), the SwinV2 family and the bf16 operand modes run the fp16-plane form of the
 * same term count instead (mdpt_get_class_f8 tells). Changes the packed-weight layout and the workspace
 * plan: call it after mdpt_create and BEFORE mdpt_packed_bytes / mdpt_finalize / mdpt_workspace_bytes (bound pointers are kept).
 * mdpt_get_class_passes reads the current assignment; mdpt_default_mixed_passes fills the table MDPT_PREC_MIXED uses. */
#define MDPT_PASSES_2F8 4 /* A_hi W_hi on fp16 planes + A_lo W_hi on fp8 planes */
#define MDPT_PASSES_3F8 5 /* A_hi W_hi on fp16 planes + A_lo W_hi + A_hi W_lo on fp8 planes */
int mdpt_set_class_passes(mdpt_handle* h, int32_t op_class, int32_t passes);
int mdpt_get_class_passes(const mdpt_handle* h, int32_t op_class, int32_t* passes);
int mdpt_get_class_f8(const mdpt_handle* h, int32_t op_class, int32_t* on); /* 1: the class's cross terms really run on fp8 planes */
void mdpt_default_mixed_passes(int32_t passes[MDPT_NUM_CLASSES]);                      /* the Depth-Anything families */
void mdpt_default_mixed_passes_for(int32_t family, int32_t passes[MDPT_NUM_CLASSES]);  /* per MDPT_FAMILY_*: the MiDaS v3.1 families keep three
                                                                                          terms on the decoder's whole projection path. Round 6: the
                                                                                          decoder classes name the fp8 forms (MDPT_PASSES_*F8); BEiT adds
                                                                                          fc1 and fc2 at 3 and fusion_in at 2F8 (margin under either rounding
                                                                                          of the fp16 weight scale, profiles/r06_beitl_class_budget.txt) */
void mdpt_default_mixed_passes_r05(int32_t family, int32_t passes[MDPT_NUM_CLASSES]);  /* the 16-bit-plane table of round 5: what MDPT_PREC_MIXED gives a class
                                                                                          of a configuration that cannot run the fp8 forms (mdpt_get_class_f8) */
/* Token-mean compensation of the weight rounding (fp16 operand modes; on by default in MDPT_PREC_MIXED, available in MDPT_PREC_FP16): a
 * single-pass Linear of the encoder (QKV, proj, fc1, fc2) computes A fp16(W)^T; what the weight rounding loses is dominated by the part all
 * tokens of an image share, mean_t(A) (W - fp16(W))^T, which two small kernels turn into a per-image bias table the GEMM epilogue adds
 * (transformer_block.py:160,168, misc_helpers.py:111-115 restated with that term). Same call-order rule as mdpt_set_class_passes.
 * on: 0 off, 1 all four classes, or a mask (1 << MDPT_CLASS_QKV) | (1 << MDPT_CLASS_PROJ) | (1 << MDPT_CLASS_FC1) | (1 << MDPT_CLASS_FC2) of the classes to compensate. */
int mdpt_set_weight_rounding_compensation(mdpt_handle* h, int32_t on);

/* Parameter inventory, named with the reference's converted ("new format") keys, prefixed by component:
 * "patch_embed.proj.weight", "imgencoder.stages.0.blocks.0.attn.qkv.weight", "reassemble.spatial_upx4.resample.1.weight",
 * "fusion.blocks.0.conv_reassembly.resconv_seq.1.weight", "head.proj_1ch.2.bias", ...
 * (state_dict_conversion/convert_original_state_dict_keys.py:15-86). */
int mdpt_num_weights(const mdpt_handle* h);
const char* mdpt_weight_name(const mdpt_handle* h, int index);
int mdpt_weight_shape(const mdpt_handle* h, int index, int32_t* ndim, int64_t shape[4]);

/* element types of the tensors handed to mdpt_bind_weight / mdpt_forward / mdpt_allgather */
#define MDPT_DTYPE_F32 0
#define MDPT_DTYPE_BF16 1
#define MDPT_DTYPE_F16 2

/* replaces <sub-module>.load_state_dict(...) (make_depthanythingv2_dpt.py:55-59). `dev_ptr` is a contiguous device tensor of
 * element type `dtype` (MDPT_DTYPE_*: the parameter as the caller holds it, e.g. bf16 after model.to(torch.bfloat16)) in the
 * PyTorch layout of that parameter; it is only read during mdpt_finalize(). */
int mdpt_bind_weight(mdpt_handle* h, const char* name, const void* dev_ptr, int32_t dtype, int32_t ndim, const int64_t* shape);

/* replaces model.to(device, dtype) (run_image.py:158): one-time repack of all bound weights into MFMA-friendly
 * bf16 (hi[/lo]) [N][K] panels inside the caller-provided `packed_dev` buffer (size from mdpt_packed_bytes).
 * Strict: fails with MDPT_E_MISSING if any parameter is unbound. */
int mdpt_packed_bytes(const mdpt_handle* h, size_t* bytes);
int mdpt_finalize(mdpt_handle* h, void* packed_dev, size_t bytes, void* stream);

/* Workspace (activations) needed for a batch of B images of H x W pixels. */
int mdpt_workspace_bytes(const mdpt_handle* h, int32_t B, int32_t H, int32_t W, size_t* bytes);

/* replaces DPTModel.forward (dpt_model.py:61-83): image [B,3,H,W] (RGB, normalised; element type image_dtype) -> depth [B,H,W]
 * (element type depth_dtype: the reference returns the model dtype, dpt_model.py:105-107). The patchify kernel reads the image in its
 * own dtype and the fused head epilogue writes the depth in the requested one: a bf16 model pays no cast kernels.
 * H, W multiples of patch_size_px with an even patch grid. */
int mdpt_forward(mdpt_handle* h, const void* image_bchw, int32_t image_dtype, int32_t B, int32_t H, int32_t W, void* depth_bhw,
                 int32_t depth_dtype, void* workspace, size_t workspace_bytes, void* stream);

/* Stage-level entry points == the five sub-module calls (simple_examples/internal_features.py:39-45). */
/* PatchEmbed.forward (v2_depthanything/patch_embed.py:77-99): -> tokens [B, (H/P)*(W/P), F] */
int mdpt_patch_embed(mdpt_handle* h, const void* image_bchw, int32_t B, int32_t H, int32_t W, void* tokens_bnf, void* workspace,
                     size_t workspace_bytes, void* stream);
/* DinoV2Model4Stages.forward (image_encoder_model.py:80-94): tokens [B,gh*gw,F] -> 4 x [B, 1+gh*gw, F] */
int mdpt_encoder(mdpt_handle* h, const void* tokens_bnf, int32_t B, int32_t gh, int32_t gw, void* const stage_out[4],
                 void* workspace, size_t workspace_bytes, void* stream);
/* ReassembleModel.forward (reassembly_model.py:61-94): 4 x [B,1+gh*gw,F] -> [B,C,4gh,4gw],[B,C,2gh,2gw],[B,C,gh,gw],[B,C,gh/2,gw/2] */
int mdpt_reassemble(mdpt_handle* h, const void* const stage_in[4], int32_t B, int32_t gh, int32_t gw, void* const maps_out[4],
                    void* workspace, size_t workspace_bytes, void* stream);
/* FusionModel.forward (fusion_model.py:55-80): the 4 maps above -> [B,C,8gh,8gw] */
int mdpt_fusion(mdpt_handle* h, const void* const maps_in[4], int32_t B, int32_t gh, int32_t gw, void* fused_out, void* workspace,
                size_t workspace_bytes, void* stream);
/* mdpt_encoder plus the explicit attention weights of selected blocks: what the reference's non-optimised attention exposes through its
 * nn.Softmax module (enable_optimizations=False, v2_depthanything/components/transformer_block.py:101,126-131; hooked by
 * experiments/attention_visualization.py:325-332). attn_out has num_blocks entries; every non-NULL entry receives that block's
 * softmax(q k^T / sqrt(d) [+ relative-position bias]) as fp32 [B, heads, N, N] (N = 1 + gh*gw) for the ViT / BEiT families.
 * SwinV2 (whose window attention always goes through a hookable nn.Softmax, v31_swinv2/components/windowed_attention.py:60-61,119):
 * blocks are numbered stage-major, an entry receives softmax(cosine attention * logit scale + position bias + shift mask) of every
 * window as fp32 [B * windows, heads_of_the_stage, Nw, Nw] (windows in the reference's partition order, tokens in window order).
 * mdpt_attn_probe_shape() gives the shape of a block's entry for a batch / grid. */
int mdpt_encoder_probe(mdpt_handle* h, const void* tokens_bnf, int32_t B, int32_t gh, int32_t gw, void* const stage_out[4],
                       void* const* attn_out, void* workspace, size_t workspace_bytes, void* stream);
int mdpt_attn_probe_shape(const mdpt_handle* h, int32_t B, int32_t gh, int32_t gw, int32_t block, int64_t shape[4]);
/* The same pass with, in addition or instead, the OUTPUT TOKENS of selected transformer blocks: what a forward hook on a block module of
 * the reference receives (demo_helpers/model_capture.py:54-59, used by experiments/block_norm_visualization.py:282 on
 * v2_depthanything/components/transformer_block.py:41-62; SwinV2: v31_swinv2/image_encoder_model.py:213-225). block_out has one entry
 * per block (SwinV2: stage-major); every non-NULL entry receives fp32 [B, 1 + gh*gw, F] (ViT / BEiT families, cls row first) or
 * [B, tokens of the block's stage, features of the stage] (SwinV2). attn_out and block_out may each be NULL. */
int mdpt_encoder_probe_blocks(mdpt_handle* h, const void* tokens_bnf, int32_t B, int32_t gh, int32_t gw, void* const stage_out[4],
                              void* const* attn_out, void* const* block_out, void* workspace, size_t workspace_bytes, void* stream);
/* The same pass with the per-token L2 NORMS of every block's output instead of the tokens (experiments/block_norm_visualization.py:133-147 keeps
 * block_tensor.norm(dim=-1) of the patch tokens and nothing else) - additive to ABI v6. norm_out has one entry per block (SwinV2: stage-major);
 * every non-NULL entry receives sqrt(sum x^2) over the features of each patch token of that block's fp32 output as fp32 [B, gh, gw] (ViT / BEiT
 * families, the cls token dropped) or [B, gh >> s, gw >> s] (a SwinV2 block of stage s). channel_out (may be NULL) has the same layout; a non-NULL
 * entry l receives channel channel_index[l] of the same tokens (the script's "Channel" view, tensor[0, :, :, ch]); a channel_index[l] outside
 * [0, features of the block) is MDPT_E_INVALID before anything is launched. stage_out receives the four encoder taps as with mdpt_encoder; the
 * taps, and every kernel of the pass itself, are those of mdpt_encoder. A row's norm does not depend on the batch it is part of. */
int mdpt_encoder_block_norms(mdpt_handle* h, const void* tokens_bnf, int32_t B, int32_t gh, int32_t gw, void* const stage_out[4], void* const* norm_out,
                             const int32_t* channel_index, void* const* channel_out, void* workspace, size_t workspace_bytes, void* stream);
/* FusionModel.blocks[index].forward (fusion_model.py:89-114 top-most block, :148-154 regular blocks; called one by one by
 * experiments/fusion_scaling.py:330-334): reassembly map [B,C,sh,sw] (+ the previous block's output [B,C,sh,sw]; NULL for index 3,
 * the top-most block) -> [B,C,2sh,2sw]. */
int mdpt_fusion_block(mdpt_handle* h, int32_t index, const void* reasm_in, const void* prior_in, int32_t B, int32_t sh, int32_t sw,
                      void* out, void* workspace, size_t workspace_bytes, void* stream);
/* MonocularDepthHead.forward (head_model.py:89-106): [B,C,8gh,8gw] -> [B, gh*P, gw*P] */
int mdpt_head(mdpt_handle* h, const void* fused_in, int32_t B, int32_t gh, int32_t gw, void* depth_bhw, void* workspace,
              size_t workspace_bytes, void* stream);

/* Batches of at least `min_batch` images (default 8; 0 = never) are run by mdpt_forward as two half batches, one on the caller's
 * stream and one on an internal side stream (event fork / join, no host synchronisation): the halves' kernels overlap and fill
 * each other's partially occupied last round of tiles. Results are bit-identical to the unsplit run. mdpt_workspace_bytes
 * accounts for the split. */
int mdpt_set_batch_split(mdpt_handle* h, int32_t min_batch);

/* The reference's `enable_cache` (make_*_dpt(..., enable_cache=True); v2_depthanything/components/position_encoder.py:152-227 GridCache,
 * v31_beit/components/relative_positional_encoder.py, v31_swinv2 default True; run_video.py:144 switches it on). Off (default): every forward
 * recomputes the per-grid constants - the bicubic-resized position embedding, BEiT's resized relative-position tables, SwinV2's
 * continuous-position-bias tables, the zero pads of operand planes. On: the first mdpt_forward of a (workspace, B, H, W) leaves them in the
 * workspace and the following mdpt_forward calls on the SAME workspace and shape skip the kernels that write them (same bits). The cached state is
 * dropped by a different shape on that workspace, by any stage-level call on the handle, and by mdpt_finalize. With the cache on the caller must
 * not write into the workspace between calls, and a caller that frees a workspace and allocates a new one (which may land at the same address)
 * calls mdpt_set_grid_cache(h, 1) again: setting the switch drops every cached slot (the Python engine does so on every workspace allocation). */
int mdpt_set_grid_cache(mdpt_handle* h, int32_t on);

/* Latency mode (default off). Off: every image's result is bit-identical whatever batch it is part of (the kernels that run do
 * not depend on the batch size in any way that changes the arithmetic). On: launches that are too small to fill the GPU (batch 1 of
 * the small models) may use forms that change the summation order - today the attention kernel splits the key loop over the four
 * waves of a workgroup and merges the partial softmax states (ViT-S, batch 1: +13 %) - so results can differ in the last bit from
 * the batch-invariant form. Accuracy against the fp32 oracle is unchanged. Round 4: fc2 of a small batch (long K on the small GEMM tile:
 * one serial chain of 64 K tiles per workgroup at ViT-L) splits K into two fixed halves, twice the workgroups in flight; the second half's
 * partial sums are folded in by the LayerNorm that follows (no reduction launch); the long-K 3x3 convs of the coarse decoder levels run as K
 * ranges that store partial planes plus a small finishing kernel. The splits are fixed per shape: results are reproducible run to run. */
int mdpt_set_latency_mode(mdpt_handle* h, int32_t on);

/* Non-finite propagation (default on; additive to ABI v6). The reference's forward (muggled_dpt/dpt_model.py:61-83) turns an image that holds a
 * NaN / inf into an all-NaN depth map: the value reaches every token of that image through the first attention, and torch's ReLU keeps it. The
 * kernels here would hide it (the fp16 operand converts saturate through v_med3, the ReLUs are v_max): so mdpt_forward has its im2col kernel flag
 * such images (it reads every pixel anyway) and one small launch behind the head writes their depth maps as NaN - in every arithmetic mode, the
 * other images of the batch untouched. Cost: one B-word memset and one launch per forward, both stream-ordered and graph-capturable. Off = the
 * earlier behaviour (a finite, meaningless map for such an image). mdpt_forward_bgr's uint8 source cannot hold a non-finite value; the stage-level
 * entry points (mdpt_patch_embed ...) return what their own arithmetic gives; non-finite WEIGHTS are the caller's to check. */
int mdpt_set_nonfinite_propagation(mdpt_handle* h, int32_t on);

/* PatchEmbed.prepare_image (v2_depthanything/patch_embed.py:103-145): uint8 [in_h,in_w,3] BGR on the device ->
 * [3,out_h,out_w] RGB in the element type out_dtype (MDPT_DTYPE_*: the model's dtype, what mdpt_forward takes next - no cast kernel in
 * between), antialiased-bilinear resized exactly like F.interpolate(..., antialias=True) in fp32 and normalised with the
 * given per-channel mean/std (ImageNet values for Depth-Anything, 0.5/0.5 for BEiT). The caller picks out_h/out_w with the reference's size rule (multiples of 2*patch).
 * `interpolation` = the reference's interpolation_mode argument (patch_embed.py:108,141): bilinear (its default) or bicubic; torch itself
 * rejects antialias=True for every other mode, and so does this entry point (MDPT_E_UNSUPPORTED). */
#define MDPT_INTERP_BILINEAR 0
#define MDPT_INTERP_BICUBIC 1
int mdpt_prepare_image(const void* bgr_u8_hwc, int32_t in_h, int32_t in_w, void* out_chw, int32_t out_dtype, int32_t out_h, int32_t out_w,
                       const float rgb_mean[3], const float rgb_std[3], int32_t interpolation, void* stream);

/* DPTModel.inference's device half in ONE call (dpt_model.py:87-109: prepare_image_bgr -> forward; SURVEY §8(f) row 1 "fused with patchify"):
 * uint8 [in_h,in_w,3] BGR on the device -> depth [H,W]. The patch embedding's im2col kernel computes every pixel of the [3,H,W] model tensor from
 * the uint8 image itself (the arithmetic of mdpt_prepare_image, rounded to image_dtype = the model's dtype) and stores it straight into its rows:
 * the normalised image never exists in memory, one launch and one HBM round trip fewer than mdpt_prepare_image + mdpt_forward, bit-identical to
 * that pair. One image per call (the reference's inference is per image); H, W by the reference's size rule; workspace as for mdpt_forward(B = 1). */
int mdpt_forward_bgr(mdpt_handle* h, const void* bgr_u8_hwc, int32_t in_h, int32_t in_w, int32_t image_dtype, int32_t H, int32_t W, const float rgb_mean[3],
                     const float rgb_std[3], int32_t interpolation, void* depth_hw, int32_t depth_dtype, void* workspace, size_t workspace_bytes, void* stream);

/* mdpt_forward_bgr for B frames of one size (DPTModel.inference_batch; additive to ABI v6): uint8 [B,in_h,in_w,3] BGR, packed, on the device -> depth
 * [B,H,W]. The im2col kernel takes the frame index as its grid's y dimension, so all B frames are resized, normalised and patchified in one launch.
 * Image b's map equals mdpt_prepare_image(frame b), stacked, then mdpt_forward of the batch, bit for bit, in every family, dtype and arithmetic mode
 * (latency mode included); a batch at or above the split size (mdpt_set_batch_split) runs as two halves exactly as mdpt_forward does. B = 1 is
 * mdpt_forward_bgr. Workspace as for mdpt_forward(B). */
int mdpt_forward_bgr_batch(mdpt_handle* h, const void* bgr_u8_bhwc, int32_t B, int32_t in_h, int32_t in_w, int32_t image_dtype, int32_t H, int32_t W,
                           const float rgb_mean[3], const float rgb_std[3], int32_t interpolation, void* depth_bhw, int32_t depth_dtype, void* workspace,
                           size_t workspace_bytes, void* stream);

/* mdpt_forward_bgr_batch for B frames of ANY sizes (DPTModel.inference_images; additive to ABI v6): frame b is uint8 [frames_hw[2b],
 * frames_hw[2b+1], 3] BGR at device pointer frames_u8_hwc[b]; every frame is resized to the one model tensor size H x W -> depth [B,H,W]. The
 * host arrays are read during the call only. The im2col kernel takes its frame table by value (64 frames per launch): nothing is
 * allocated or copied to the device, the call never synchronises and stays graph-capturable. Image b's map equals mdpt_prepare_image(frame b),
 * stacked, then mdpt_forward of the batch, bit for bit, in every family, dtype and arithmetic mode; a batch at or above the split size runs as
 * two halves, the second from table entry B0. Errors as mdpt_forward_bgr_batch. Workspace as for mdpt_forward(B). */
int mdpt_forward_bgr_frames(mdpt_handle* h, const void* const* frames_u8_hwc, const int32_t* frames_hw, int32_t B, int32_t image_dtype, int32_t H, int32_t W,
                            const float rgb_mean[3], const float rgb_std[3], int32_t interpolation, void* depth_bhw, int32_t depth_dtype, void* workspace,
                            size_t workspace_bytes, void* stream);

/* Crop and region inference (the reference's --crop: frame[y_slice, x_slice] before dpt_model.inference; additive to ABI v6). A box of an image is
 * a frame: the resize kernels read it where the image lies - first pixel at byte y1 * pitch + 3 * x1, rows `pitch` bytes apart - and their
 * antialias taps clip at the BOX's edges, so the result equals, bit for bit, the same call on a packed copy of the box and never depends on a pixel
 * outside it. Pitches and frame strides are in BYTES and 64-bit; boxes are x1, y1, x2, y2 in pixels, half-open (0 <= x1 < x2 <= w, 0 <= y1 < y2 <= h).
 * Nothing is copied, allocated or synchronised; everything is validated on the host before the first launch (MDPT_E_INVALID).
 *
 *   frames                         table run        pitch            frame_stride
 *   packed [B,h,w,3]               one, count B     3 w              3 h w
 *   view / box of a [B,H,W,3]      one, count B     the tensor's     the tensor's
 *   list of frames, any sizes      one per frame    3 w_b            -
 *   list of boxes of images        one per box      image b's        -
 *
 * The pitch-and-box form of mdpt_prepare_image: pitch 0 = packed (3 * in_w); H, W are the caller's, from the size rule applied to the BOX's size. */
int mdpt_prepare_image_region(const void* bgr_u8_hwc, int32_t in_h, int32_t in_w, int64_t pitch, const int32_t box_xyxy[4], void* out_chw, int32_t out_dtype,
                              int32_t out_h, int32_t out_w, const float rgb_mean[3], const float rgb_std[3], int32_t interpolation, void* stream);

/* The one-size batch read in place: frame b is uint8 [in_h,in_w,3] at bgr_u8 + b * frame_stride with rows `pitch` (>= 3 * in_w) bytes apart - one box
 * cut out of every frame of a [B,H,W,3] tensor, or a sliced view of one. One run of the frame table, one im2col launch; with pitch = 3 * in_w and
 * frame_stride = 3 * in_h * in_w it is the packed batch entry point above. frame_stride is not read when B = 1. */
int mdpt_forward_bgr_pitched(mdpt_handle* h, const void* bgr_u8, int32_t B, int32_t in_h, int32_t in_w, int64_t pitch, int64_t frame_stride,
                             int32_t image_dtype, int32_t H, int32_t W, const float rgb_mean[3], const float rgb_std[3], int32_t interpolation, void* depth_bhw,
                             int32_t depth_dtype, void* workspace, size_t workspace_bytes, void* stream);

/* B regions in one batched forward (DPTModel.inference_regions): region b is the box boxes_xyxy[4b .. 4b+3] of the uint8 [images_hw[2b],
 * images_hw[2b+1], 3] BGR image at device pointer images_u8_hwc[b], whose rows are images_pitch[b] bytes apart (images_pitch NULL = every image
 * packed). Images may repeat and boxes may overlap; every region is resized to the one model tensor size H x W -> depth [B,H,W]. The host arrays are
 * read during the call only; tables go 64 regions per im2col launch and a batch at or above the split size runs as two halves, the second from table
 * entry B0, as the per-frame entry point above does. Region b's map equals the single-image entry point on a packed copy of its box, bit for bit.
 * 1 <= B <= 65535. Workspace as for mdpt_forward(B). */
int mdpt_forward_bgr_regions(mdpt_handle* h, const void* const* images_u8_hwc, const int32_t* images_hw, const int64_t* images_pitch, const int32_t* boxes_xyxy,
                             int32_t B, int32_t image_dtype, int32_t H, int32_t W, const float rgb_mean[3], const float rgb_std[3], int32_t interpolation,
                             void* depth_bhw, int32_t depth_dtype, void* workspace, size_t workspace_bytes, void* stream);

/* Depth post-processing on the device (reference muggled_dpt/demo_helpers/postprocess.py and
 * run_3dviewer.py:576-590). All buffers are device pointers; `minmax` is a 2-float device buffer {min, max} and
 * `scratch8` 8 bytes of device scratch - nothing is read back to the host, nothing synchronises.
 *   mdpt_post_minmax ............ data.min(), data.max() of an fp32 array (normalize_01, postprocess.py:72-73)
 *   mdpt_post_scale_prediction .. F.interpolate(pred[:, None], size=(out_h, out_w), mode="bilinear") (postprocess.py:22-29);
 *                                 minmax_out != NULL also reduces min/max of the OUTPUT in the same pass
 *   mdpt_post_normalize ......... mode MDPT_POST_F32: (x - min) / (max - min) -> fp32            (postprocess.py:74)
 *                                 mode MDPT_POST_U8:  (255 * norm).byte() -> uint8 (truncation)     (postprocess.py:91)
 *                                 mode MDPT_POST_U24: round(16777215 * norm) -> BGRA uint8x4, B/G/R = low/mid/high byte,
 *                                                     alpha 0; lossy != 0 keeps only the high byte (run_3dviewer.py:579-590)
 *                                 minmax == NULL skips the normalisation (metric models, run_3dviewer.py:577-578) */
#define MDPT_POST_F32 0
#define MDPT_POST_U8 1
#define MDPT_POST_U24 2
int mdpt_post_minmax(const void* in_f32, size_t count, void* minmax_out, void* scratch8, void* stream);
int mdpt_post_scale_prediction(const void* in_bhw_f32, int32_t B, int32_t in_h, int32_t in_w, void* out_bhw_f32, int32_t out_h,
                               int32_t out_w, void* minmax_out, void* scratch8, void* stream);
int mdpt_post_normalize(const void* in_f32, size_t count, const void* minmax, void* out, int32_t mode, int32_t lossy, void* stream);

/* Per-image display tail (additive to ABI v6): the per-frame loop of the reference's video demo (run_video.py:348-361: scale_prediction ->
 * convert_to_uint8 -> optional 255 - x -> histogram_equalization -> colormap LUT) over a batch, every image with its own min/max, histogram and
 * LUT, nothing read back to the host. Image b's result equals the per-frame composition on image b alone, bit for bit; a NaN map gives that image
 * what MDPT_POST_U8 gives it (all 0 before the reverse) and touches no other image. Buffers (device):
 *   parts  [B, MDPT_POST_SEG_PARTS, 2] uint32, the per-image min/max partials mdpt_post_minmax_seg leaves for mdpt_post_u8_hist_seg
 *   hist   [B, 256] uint32 counts, ACCUMULATED into (zero it first, e.g. through mdpt_post_minmax_seg's hist_clear)
 *   lut    [B, 256] uint8 equalization LUTs; cmap_bgr [256, 3] uint8 BGR (a 1x256x3 colormap LUT)
 *   mdpt_post_minmax_seg ...... out_bhw_f32 == NULL: per-image min/max of in_bhw ([B,in_h,in_w], dtype in_dtype = MDPT_DTYPE_*);
 *                               else mdpt_post_scale_prediction's bilinear resize of each image to out_h x out_w, rounded to in_dtype (the map
 *                               scale_prediction returns), stored as fp32, and the per-image min/max of that. hist_clear != NULL: zeroes [B,256]
 *   mdpt_post_u8_hist_seg ..... (255 * normalize_01(image b)).byte() per image (MDPT_POST_U8 arithmetic, image b's min/max), reverse != 0: 255 - x,
 *                               -> out_u8 [B,count]; hist != NULL also counts the result into hist (LDS-private bins, integer atomics)
 *   mdpt_post_histogram ....... 256-bin histogram per image of a uint8 [B,count] batch, accumulated into hist
 *   mdpt_post_equalize_lut .... the equalization LUT of every image (demo_helpers/postprocess.py:107-145). bin_of_value == NULL: cv2.equalizeHist
 *                               (fp32, round half to even). Otherwise the thresholded branch: bin_of_value = 256 int32 on the device, the bin
 *                               np.histogram(x, 1 + max - min, range=(min, max)) puts value v in (-1: outside), LUT built in fp64 as numpy does
 *   mdpt_post_colorize ........ out = cmap_bgr[eq_lut[b][x]] as [B,count,3] BGR (channels 3), or eq_lut[b][x] as [B,count] (channels 1);
 *                               eq_lut == NULL: identity, cmap_bgr == NULL: gray (cv2.cvtColor GRAY2BGR) */
#define MDPT_POST_SEG_PARTS 64
int mdpt_post_minmax_seg(const void* in_bhw, int32_t in_dtype, int32_t B, int32_t in_h, int32_t in_w, void* out_bhw_f32, int32_t out_h, int32_t out_w,
                         void* parts, void* hist_clear, void* stream);
int mdpt_post_u8_hist_seg(const void* in_bhw, int32_t in_dtype, int32_t B, size_t count, const void* parts, int32_t reverse, void* out_u8, void* hist,
                          void* stream);
int mdpt_post_histogram(const void* in_u8, int32_t B, size_t count, void* hist, void* stream);
int mdpt_post_equalize_lut(const void* hist, int32_t B, const void* bin_of_value, int32_t min_value, int32_t max_value, void* lut_out, void* stream);
int mdpt_post_colorize(const void* in_u8, int32_t B, size_t count, const void* eq_lut, const void* cmap_bgr, int32_t channels, void* out, void* stream);

/* The same display tail for B images of DIFFERENT sizes (postprocess.scale_prediction_images / depth_to_color_images; additive to ABI v6).
 * Image i is in[i] (device pointer) of hw[2i] x hw[2i+1] elements; outputs are packed in image order (image i's output starts where image
 * i-1's ends). parts / hist / eq_lut are [B, ...] as above. The host arrays are read during the call only; every kernel takes its image table
 * by value, so each of the three is one launch per 32 images, and image i's result equals the uniform entry point on image i
 * alone, bit for bit:
 *   mdpt_post_minmax_images .... mdpt_post_minmax_seg per image; out_f32 != NULL: image i resized to out_hw[2i] x out_hw[2i+1] into out_f32
 *   mdpt_post_u8_hist_images ... mdpt_post_u8_hist_seg per image (in[i]: the map mdpt_post_minmax_images measured, hw its size)
 *   mdpt_post_colorize_images .. mdpt_post_colorize per image of a packed uint8 input (in_u8), hw the images' sizes */
int mdpt_post_minmax_images(const void* const* in, const int32_t* in_hw, int32_t in_dtype, int32_t B, void* out_f32, const int32_t* out_hw, void* parts,
                            void* hist_clear, void* stream);
int mdpt_post_u8_hist_images(const void* const* in, const int32_t* hw, int32_t in_dtype, int32_t B, const void* parts, int32_t reverse, void* out_u8,
                             void* hist, void* stream);
int mdpt_post_colorize_images(const void* in_u8, const int32_t* hw, int32_t B, const void* eq_lut, const void* cmap_bgr, int32_t channels, void* out,
                              void* stream);

/* Still-image display tail and 24-bit edge alpha on the device (additive to ABI v6): the per-image loop of the reference's still-image demo
 * (run_image.py:185-195 display, :323-343 threshold / equalization / colormap, :350-358 .npy save) and the alpha channel of its 3D viewer
 * (run_3dviewer.py:455-505 edge mask, :576-593 packing). Uniform batches of B images of H x W; nothing is read back, nothing synchronises.
 * Buffers (device): parts as above; coef [B, 4] fp64 plane {nx, ny, nz, d} (plane = -(d + nx x + ny y) / nz); vparts [B, MDPT_POST_SEG_PARTS, 2]
 * fp64 {min, max} partials; mag [B, H, W] fp32; mag_max [B] uint32 (fp32 bits); sample_xy int32 (x, y) pairs, [N, 2] or [B, N, 2].
 *   mdpt_post_display_prep ... remove_inf(scale_prediction(x)) per image: bilinear resize to out_h x out_w (a copy when the size is unchanged),
 *                              rounded to in_dtype, +-inf -> 0, stored in in_dtype at out_bhw; parts = its per-image min/max; hist_clear zeroes [B,256]
 *   mdpt_post_plane_fit ...... one workgroup per image (demo_helpers/plane_fit.py): z at the sample points (parts != NULL: of normalize_01 of the
 *                              map, evaluated in in_dtype as torch does), the 3x3 Gram matrix of the centred samples (x / y means (W-1)/2,
 *                              (H-1)/2) in fp64, its smallest eigenvector by Jacobi -> coef. Points are clamped into the map. A constant map
 *                              gives the constant plane.
 *   mdpt_post_plane_eval ..... the plane images of coef -> out_f32 [B,H,W]
 *   mdpt_post_plane_minmax ... v = normalize_01(x) - factor * plane in fp64 (parts, coef of the same map) -> vparts
 *   mdpt_post_threshold ...... t = clip((normalize_01(v) - thresh_min) / max(0.001, thresh_max - thresh_min), 0, 1) in fp64. mode MDPT_POST_U8:
 *                              round-half-even(255 t) -> out uint8 [B,H,W], hist != NULL counts it (zero it first); reverse must be 0 (255 - x
 *                              comes after the equalization: reverse the colormap instead). mode MDPT_POST_F32: t, or 1 - t with reverse -> fp32
 *   mdpt_post_edge_mag ....... the viewer's 5x5 Gaussian blur (blur_weights: blur_ksize^2 fp32 on the HOST, read during the call; odd size up to 15)
 *                              and 3x3 Sobel, both with reflect padding, mag = sqrt(dx^2 + dy^2) -> mag_f32 and its per-image max -> mag_max
 *                              (cleared by the call). parts != NULL: of normalize_01 of the map (fp32). Sides must be at least max(2, pad + 1).
 *   mdpt_post_edge_mask ...... ~round(255 mag / max) -> uint8 [B,count]; a flat map (max 0) gives 255 everywhere
 *   mdpt_post_pack_u24_alpha . mdpt_post_normalize(MDPT_POST_U24) per image (parts: its min/max; NULL: metric, as is) with the alpha byte in the same
 *                              pass: the edge byte of mag_f32 / mag_max, or mask_u8 ([count], or [B,count] with mask_per_image), or 0 */
int mdpt_post_display_prep(const void* in_bhw, int32_t in_dtype, int32_t B, int32_t in_h, int32_t in_w, void* out_bhw, int32_t out_h, int32_t out_w,
                           void* parts, void* hist_clear, void* stream);
int mdpt_post_plane_fit(const void* in_bhw, int32_t in_dtype, int32_t B, int32_t H, int32_t W, const void* parts, const void* sample_xy, int32_t num_samples,
                        int32_t xy_per_image, void* coef_out, void* stream);
int mdpt_post_plane_eval(const void* coef, int32_t B, int32_t H, int32_t W, void* out_f32, void* stream);
int mdpt_post_plane_minmax(const void* in_bhw, int32_t in_dtype, int32_t B, int32_t H, int32_t W, const void* parts, const void* coef, double factor,
                           void* vparts, void* stream);
int mdpt_post_threshold(const void* in_bhw, int32_t in_dtype, int32_t B, int32_t H, int32_t W, const void* parts, const void* coef, double factor,
                        const void* vparts, double thresh_min, double thresh_max, int32_t mode, int32_t reverse, void* out, void* hist, void* stream);
int mdpt_post_edge_mag(const void* in_bhw_f32, int32_t B, int32_t H, int32_t W, const void* parts, const float* blur_weights, int32_t blur_ksize,
                       void* mag_f32, void* mag_max, void* stream);
int mdpt_post_edge_mask(const void* mag_f32, const void* mag_max, int32_t B, size_t count, void* out_u8, void* stream);
int mdpt_post_pack_u24_alpha(const void* in_bhw_f32, int32_t B, size_t count, const void* parts, int32_t lossy, const void* mag_f32, const void* mag_max,
                             const void* mask_u8, int32_t mask_per_image, void* out_bgra, void* stream);

/* Depth masking on the device (additive to ABI v6): the reference's background removal by depth (experiments/depth_masking.py: display :189-199,
 * :314-332; save :341-361), nothing read back, nothing synchronised. The map side is the still-image chain above (mdpt_post_display_prep ->
 * mdpt_post_plane_fit -> mdpt_post_plane_minmax: parts, coef, vparts of the prepared map); n = normalize_01(normalize_01(x) - factor * plane) in fp64,
 * mask = 255 where thresh_min <= value <= thresh_max (a NaN compares false: 0), 255 - mask with invert. cv2.resize(INTER_LINEAR) is restated per
 * axis: p = float((d + 0.5) * (1 / (out / in)) - 0.5), s = floor(p), a = p - s (fp32); s < 0 -> s = 0, a = 0; s >= in - 1 -> s = in - 1, a = 0.
 *   mdpt_post_mask_display ........ uniform batch at the display size H x W: mask of n -> mask_out uint8 [B,H,W]; composite_out uint8 [B,H,W,3] =
 *                                   cv2.resize of photo b (images_bgr uint8 [B,image_h,image_w,3], CV_8U: weights round(2048 w), integer sums,
 *                                   (v + 2^21) >> 22 - cv2's scalar fixed-point path; its SIMD / IPP paths may differ by 1) where the mask is 255,
 *                                   CheckerPattern() (169 / 214, 32-px tiles, centred by BORDER_WRAP) where it is 0
 *   mdpt_post_mask_cutout_images .. B photos of any sizes, each cut out by its own prepared map: maps[k] (map_hw[2k] x map_hw[2k+1], map_dtype) with
 *                                   its parts[k] / coef[k] / vparts[k] (device pointers of ONE image's rows), photo images[k] (device, uint8
 *                                   image_hw[2k] x image_hw[2k+1] x 3 BGR): s = cv2.resize(n, photo size) in fp64 (CV_64F: fp32 weights, fp64
 *                                   sums, rows first), its mask -> out_mask + out_offsets[k] (pixels), BGRA (BGR AND mask, alpha = mask) ->
 *                                   out_bgra + 4 * out_offsets[k] (4-byte aligned). Host arrays are read during the call only; one launch per
 *                                   32 photos. */
int mdpt_post_mask_display(const void* in_bhw, int32_t in_dtype, int32_t B, int32_t H, int32_t W, const void* parts, const void* coef, double factor,
                           const void* vparts, double thresh_min, double thresh_max, int32_t invert, const void* images_bgr, int32_t image_h, int32_t image_w,
                           void* mask_out, void* composite_out, void* stream);
int mdpt_post_mask_cutout_images(const void* const* maps, const int32_t* map_hw, int32_t map_dtype, const void* const* parts, const void* const* coef,
                                 const void* const* vparts, double factor, const void* const* images, const int32_t* image_hw, const int64_t* out_offsets,
                                 int32_t B, double thresh_min, double thresh_max, int32_t invert, void* out_bgra, void* out_mask, void* stream);

/* Block norm tiles on the device (additive to ABI v6): BlockData.__init__ of the reference's experiments/block_norm_visualization.py:137-147 and the
 * nearest-neighbour enlargement of its display (:207-233) for L maps (norms or channel planes, maps[l] = device fp32 [B, map_hw[2l], map_hw[2l+1]]) of
 * B images at once: every (map, image) is normalised by its OWN min / max in fp32, one IEEE operation per step as numpy does it -
 * u8 = round_half_even(((n - min) / (max - min)) * 255) - and written to tiles_u8 [L, B, H, W] at (y, x) from cell (y / (H / h), x / (W / w)); H and
 * W must be whole multiples of every map's sides (what SwinV2's stages give; every nearest rule agrees there). minmax_f32 [L, B, 2] receives each
 * map's {min, max}. A constant map (0 / 0) and a map holding a NaN (min = max = NaN) give an all-zero tile, where the reference's NaN -> uint8
 * conversion is undefined. map_hw and maps are host arrays read during the call only; one launch per 32 maps; nothing is read back. */
int mdpt_post_block_norm_tiles(const void* const* maps, const int32_t* map_hw, int32_t L, int32_t B, int32_t H, int32_t W, void* tiles_u8, void* minmax_f32,
                               void* stream);

/* Depth-to-mesh on the device (additive to ABI v6): the client half of the reference's 3D viewer, its "Save 3D Model" - JavaScript on the CPU there.
 * frames_bgra = uint8 [B,H,W,4] as mdpt_post_pack_u24_alpha writes them (bytes 0..2 the low / mid / high byte of the 24-bit depth, byte 3 alpha),
 * 4-byte aligned. Nothing is read back, nothing synchronises.
 *   mdpt_post_mesh_grid ........... host arithmetic only, 3dviewer/mesh.js:184-200: t = max(target_faces, 2), tv = round(t / 2 + sqrt(t)),
 *                                   rx = sqrt(tv w / h), ry = rx / (w / h), nx = max(round(rx), 2), ny = max(round(ry), 2) in double, round =
 *                                   Math.round (halves toward +inf). Vertex (row r, col c) = index c + r nx at (c 2 / (nx - 1) - 1, 1 - r 2 / (ny - 1)).
 *   mdpt_post_mesh_scratch_bytes .. the device scratch one mdpt_post_mesh call of B images on an nx x ny grid needs
 *   mdpt_post_mesh ................ per vertex (shaders.js:185-205, 212-252; vertex_xy_f64 = device fp64 [nx ny, 2] replaces the grid's coordinates,
 *                                   NULL: the grid's own): uv = ((x + 1) / 2, (y + 1) / 2); a bilinear sample of the frame flipped vertically
 *                                   (index.html:1067-1070) at clamp01(uv) * (W - 1, H - 1), taps floor and min(floor + 1, side - 1); depth taps are
 *                                   u24 / 2^24, alpha taps the bytes; kept if alpha >= edge_threshold * 255; depth = a + b d (is_metric) or
 *                                   1 / (a + b d) (index.html:1179-1188); xyz = (depth x x_scale tan_half_fov, depth y y_scale tan_half_fov, -depth).
 *                                   All of it in fp64, rounded to fp32 once. Faces (mesh.js:207-229): cell (r, c) in vertex order gives
 *                                   [v, v + nx, v + nx + 1] and [v, v + nx + 1, v + 1]; MDPT_MESH_POINTS: [i] per vertex. Filtering
 *                                   (mesh.js:330-371): kept vertices keep their order and are renumbered from 0; a face is kept if all its vertices
 *                                   are, keeps its order and takes the new indices. Outputs are full-capacity slabs with each image's kept entries
 *                                   packed at the front (the rest is left as it was): xyz_f32 [B, nx ny, 3], uv_f32 [B, nx ny, 2], faces_u32
 *                                   [B, 2 (nx - 1)(ny - 1), 3] (points: [B, nx ny, 1]), counts_i32 [B, 2] = {kept vertices, kept faces},
 *                                   bounds_f32 [B, 2, 3] = {min xyz, max xyz} of the kept vertices (save_gltf.js:16-25; none kept: +1e6 / -1e6).
 *                                   Order-preserving and bit-deterministic; five launches (four for points).
 * Two deviations: the 24-bit depth VALUE is interpolated (the JavaScript interpolates the three bytes separately and truncates each, which is
 * garbage across a byte carry such as 0x00FFFF | 0x010000), and real bounds are not clamped to +-1e6. Grids need sides of at least 2 and fewer
 * than 2^31 vertices and faces. */
#define MDPT_MESH_TRIANGLES 0
#define MDPT_MESH_POINTS 1
int mdpt_post_mesh_grid(int32_t w, int32_t h, double target_faces, int32_t* nx, int32_t* ny);
int mdpt_post_mesh_scratch_bytes(int32_t B, int32_t nx, int32_t ny, size_t* bytes);
int mdpt_post_mesh(const void* frames_bgra, int32_t B, int32_t H, int32_t W, int32_t nx, int32_t ny, const void* vertex_xy_f64, double a, double b,
                   double tan_half_fov, double x_scale, double y_scale, double edge_threshold, int32_t is_metric, int32_t mode, void* xyz_f32,
                   void* uv_f32, void* faces_u32, void* counts_i32, void* bounds_f32, void* scratch, size_t scratch_bytes, void* stream);

/* Tiled high-resolution inference on the device (additive to ABI v6): the depth maps of T overlapping tiles of one H x W photo (what
 * mdpt_forward_bgr_regions returns for the tiles' boxes) put together into one fp32 map at the photo's resolution. Every forward of a relative-depth
 * model has its own unknown scale and shift (the reference's .readme_assets/results_explainer.md, "Results are scene-specific!"); its "Fitting to
 * (more) known data" names a least-squares fit of the two terms and has no code for it. Here the whole photo inferred once at model size is the
 * guide (gh x gw, covering the photo), every tile is fitted to the guide over its own box, and the fitted tiles are feather-blended. fp64
 * arithmetic, nothing contracted, rounded to fp32 once; nothing is read back, nothing synchronises; both calls are bit-deterministic.
 * A tile is an mdpt_tile record: its map (device pointer, h x w elements of map_dtype) and its half-open pixel box (x1, y1, x2, y2), bw = x2 - x1,
 * bh = y2 - y1. The kernels read the table from DEVICE memory (tiles_dev: the caller's upload of the T records, 8-byte aligned), so T is not bounded
 * by a kernel's arguments; tiles_host is the same table on the host, read during the call for the argument checks only.
 *   mdpt_post_tile_scratch_bytes .. the device scratch mdpt_post_tile_fit needs for this table (the partial sums)
 *   mdpt_post_tile_fit ............ one sample per tile-map pixel (j, i): x = m[j, i]; y = the guide sampled bilinearly (fp64 weights, rows first)
 *                                   at u = X gw / W - 0.5, v = Y gh / H - 0.5 clamped to the guide, (X, Y) = (x1 + (i + 0.5) bw / w,
 *                                   y1 + (j + 0.5) bh / h) the pixel's centre in the photo; a sample whose x or y is not finite is skipped.
 *                                   sums_f64 [T, 6] = {n, Sx, Sy, Sxx, Sxy, Syy}: every workgroup reduces a fixed chunk of 2048 samples with a
 *                                   fixed tree, a second launch adds each tile's partials in chunk order (no float atomics, no workgroup waits for
 *                                   another). fit_f64 [T, 2] = {s, t}: var = n Sxx - Sx^2, s = (n Sxy - Sx Sy) / var, t = (Sy - s Sx) / n. A
 *                                   degenerate tile (n < 2, var <= 0, s not finite or <= 0) gets s = 0, t = Sy / n, the guide's mean; n == 0
 *                                   gives t = 0 and marks the tile empty (sums[t][0] == 0). T <= 65535.
 *   mdpt_post_tile_blend .......... out_f32 [H, W]: per pixel, over the tiles whose box holds it, in table order, skipping empty tiles (sums_f64
 *                                   != NULL: n == 0): out = (float)(sum w z / sum w), z = s val + t (fit_f64 == NULL: s = 1, t = 0), val =
 *                                   cv2.resize(map, (bw, bh)) at (Y - y1, X - x1) by the CV_64F rule of the depth masking block above (one change: a
 *                                   lerp of two equal taps is that tap, so constant tiles blend to exactly their constant; finite taps move by at
 *                                   most the rounding of the weights, equal infinite taps give that infinity under both rules), w = wx wy,
 *                                   wx = min(1, (dx + 1) / (feather + 1)) with dx the distance in pixels to the nearer of the tile's left and
 *                                   right edge columns - an edge on the photo's border does not count, so the photo's own border has no ramp -
 *                                   and wy likewise. A pixel no tile covers is NaN; a z that is not finite propagates. feather >= 0, finite. The
 *                                   photo must need fewer than 2^24 blocks of 64 x 16 pixels, a tile map fewer than 2^24 chunks.
 * Both calls check on the host that every box lies inside the photo, that sizes are positive and that pointers are aligned (maps to their
 * element, the fp64 buffers to 8 bytes, out_f32 to 4), and launch nothing otherwise. */
typedef struct mdpt_tile { const void* map; int32_t h, w; int32_t x1, y1, x2, y2; } mdpt_tile;
int mdpt_post_tile_scratch_bytes(const mdpt_tile* tiles_host, int32_t T, size_t* bytes);
int mdpt_post_tile_fit(const mdpt_tile* tiles_host, const void* tiles_dev, int32_t T, int32_t map_dtype, const void* guide, int32_t guide_dtype,
                       int32_t guide_h, int32_t guide_w, int32_t H, int32_t W, void* fit_f64, void* sums_f64, void* scratch, size_t scratch_bytes,
                       void* stream);
int mdpt_post_tile_blend(const mdpt_tile* tiles_host, const void* tiles_dev, int32_t T, int32_t map_dtype, int32_t H, int32_t W, const void* fit_f64,
                         const void* sums_f64, double feather, void* out_f32, void* stream);

/* True depth from ground truth on the device (additive to ABI v6): P predictions aligned to measured depth maps that are partly valid and at their
 * own resolutions, scored with the standard depth metrics, and mapped to true depth. A relative-depth model returns inverse depth with an unknown
 * scale and shift per image; the reference's .readme_assets/results_explainer.md gives depth = 1 / (A V + B) ("True depth from DPT result") and, under
 * "Fitting to (more) known data", names a least-squares fit of A and B and the matching of the ground truth's median and spread, with code for
 * neither. fp64 arithmetic, nothing contracted, results rounded once; nothing is read back, nothing synchronises; every call is bit-deterministic
 * (fixed chunks of 2048 truth pixels reduced with a fixed tree and added in chunk order by the next launch; integer atomics for the select's counts
 * only; no workgroup waits for or reads another), and a pair's results do not depend on the other pairs of the call.
 * A pair is an mdpt_depth_pair record: pred (device pointer, ph x pw elements of pred_dtype), truth (fp32, H x W), valid (uint8, H x W, or NULL:
 * every pixel). Pairs of one call may all differ in size; H W < 2^31. The kernels read the table from DEVICE memory (pairs_dev: the caller's upload
 * of the P records, 8-byte aligned); pairs_host is the same table on the host, read during the call for the argument checks only. P <= 65535.
 * THE SAMPLE RULE, shared by fit and metrics: one sample per TRUTH pixel (Y, X). v = the prediction sampled bilinearly (fp64 weights, rows first)
 * at u = (X + 0.5) pw / W - 0.5, w = (Y + 0.5) ph / H - 0.5 clamped to the map (the tile fit's resampler with the roles swapped). t = 1 / truth
 * in MDPT_ALIGN_INVERSE space, t = truth in MDPT_ALIGN_DEPTH space (metric heads). The sample counts if truth is finite and > 0, tmin <= truth <=
 * tmax (-inf / +inf: no bound), valid is NULL or non-zero there, and v is finite.
 *   mdpt_post_align_scratch_bytes .. the device scratch fit and metrics need for this table (partial sums, the select's bins and state)
 *   mdpt_post_align_fit ............ fit_f64 [P, 2] = {A, B} with t ~ A v + B, sums_f64 [P, 6].
 *                                    MDPT_ALIGN_LSTSQ: sums = {n, Sv, St, Svv, Svt, Stt}; var = n Svv - Sv^2, A = (n Svt - Sv St) / var,
 *                                    B = (St - A Sv) / n, the tile fit's scheme and solve rule: a degenerate pair (n < 2, var <= 0, A not finite
 *                                    or <= 0) gets A = 0, B = St / n; n == 0 gives B = 0. Two launches.
 *                                    MDPT_ALIGN_MEDIAN (the explainer's "median and spread", MiDaS's training normalisation), on the float32
 *                                    roundings v32, t32 of the samples: med(x) the exact median, for even n ((double)lo + (double)hi) 0.5;
 *                                    mad(x) = (1 / n) sum |x - med(x)| in fp64; A = mad(t) / mad(v), B = med(t) - A med(v); mad(v) == 0 or an A
 *                                    that is not finite or <= 0 gives A = 0, B = med(t); n == 0 gives B = 0 and sums of zero. sums = {n, med v,
 *                                    med t, mad v, mad t, 0}. The median is an exact radix select on order-preserving 32-bit keys of the floats
 *                                    (sign flip; -0.0 sorts before +0.0), 8 bits a pass: a per-pair digit histogram (LDS bins, integer atomics,
 *                                    flushed with global integer atomics) and a one-workgroup-per-pair select that narrows the prefix of both
 *                                    middle ranks, (n - 1) / 2 and n / 2; v and t go through the same launches; the samples are recomputed in
 *                                    every pass, nothing per pixel is stored. Eleven launches: clear, 4 x (histogram, select), deviation, solve.
 *   mdpt_post_align_metrics ........ metrics_f64 [P, MDPT_ALIGN_NUM_METRICS] over the same samples, two launches. q = A v + B (fit_f64 == NULL:
 *                                    A = 1, B = 0, which scores a metric head as it is); aligned depth d = 1 / q in INVERSE space, d = q in
 *                                    DEPTH space; a sample whose q is not > 0 is counted in n_bad and left out. With g = truth, over the
 *                                    n - n_bad scored samples: {n, n_bad, AbsRel mean |d - g| / g, SqRel mean (d - g)^2 / g, RMSE, RMSE-log
 *                                    sqrt(mean (ln d - ln g)^2), log10 mean |log10 d - log10 g|, delta1, delta2, delta3 the share of samples with
 *                                    max(d / g, g / d) below 1.25, 1.25^2, 1.25^3, SILog 100 sqrt(mean(e^2) - mean(e)^2), e = ln d - ln g (a
 *                                    difference below zero by rounding counts as zero)}. n - n_bad == 0 gives NaN for the nine metrics.
 *   mdpt_post_align_apply .......... out_f32: pair p's H x W map (the record's H, W are the OUTPUT size here; truth and valid are not read and may
 *                                    be NULL) at out_f32 + out_offsets[p] elements (the offsets on the host for the checks and, the same int64
 *                                    values, uploaded to the device, 8-byte aligned). Per output pixel: v by the sample rule's resampler,
 *                                    q = A v + B (fit_f64 == NULL: A = 1, B = 0), INVERSE: 1 / q, and +inf where q <= 0; DEPTH: q; then clamped to
 *                                    [dmin, dmax] where those are finite (-inf / +inf: no clamp), rounded to fp32 once. A v that is not finite
 *                                    propagates through the arithmetic (NaN stays NaN). One launch: resize, affine map and reciprocal fused.
 * Every call checks on the host that sizes are positive, that H W < 2^31, that pointers are aligned (predictions to their element, truth and
 * out_f32 to 4 bytes, the table, the fp64 buffers, the offsets and the scratch to 8), that tmin <= tmax and dmin <= dmax (no NaN), and launches
 * nothing otherwise. */
#define MDPT_ALIGN_INVERSE 0
#define MDPT_ALIGN_DEPTH 1
#define MDPT_ALIGN_LSTSQ 0
#define MDPT_ALIGN_MEDIAN 1
#define MDPT_ALIGN_NUM_METRICS 11
typedef struct mdpt_depth_pair { const void* pred; int32_t ph, pw; const void* truth; const void* valid; int32_t H, W; } mdpt_depth_pair;
int mdpt_post_align_scratch_bytes(const mdpt_depth_pair* pairs_host, int32_t P, size_t* bytes);
int mdpt_post_align_fit(const mdpt_depth_pair* pairs_host, const void* pairs_dev, int32_t P, int32_t pred_dtype, int32_t space, int32_t method, double tmin,
                        double tmax, void* fit_f64, void* sums_f64, void* scratch, size_t scratch_bytes, void* stream);
int mdpt_post_align_metrics(const mdpt_depth_pair* pairs_host, const void* pairs_dev, int32_t P, int32_t pred_dtype, int32_t space, double tmin,
                            double tmax, const void* fit_f64, void* metrics_f64, void* scratch, size_t scratch_bytes, void* stream);
int mdpt_post_align_apply(const mdpt_depth_pair* pairs_host, const void* pairs_dev, int32_t P, int32_t pred_dtype, int32_t space, const void* fit_f64,
                          const int64_t* out_offsets_host, const void* out_offsets_dev, double dmin, double dmax, void* out_f32, void* stream);

/* Photo-guided depth upsampling on the device (additive to ABI v6): He & Sun's fast guided filter with the uint8 BGR photo as the guide, for the
 * step that every route above takes bilinearly - a map of about model size brought back to the photo's size - so that depth edges follow the photo's
 * edges instead of becoming ramps. P pairs of any sizes in one call, six launches whatever P is, nothing read back, nothing synchronises,
 * bit-deterministic, every pair independent of the others in the call. A pair is an mdpt_guided_pair record: the h x w map (map_dtype), the photo of
 * H x W pixels (H >= h, W >= w) whose rows start `pitch` bytes apart (pitch >= 3 W; no alignment is asked: the photo is read byte by byte, in place),
 * the fp32 H x W output (4-byte aligned), and scratch_off, the byte offset of the pair's own scratch inside `scratch` (a multiple of 8; the pair
 * needs mdpt_post_guided_scratch_bytes of its record alone from there, and the regions of a call must not overlap). The table is passed twice:
 * pairs_dev in DEVICE memory (8-byte aligned), pairs_host the same records on the host, read during the call for the argument checks only.
 * All arithmetic is fp64, nothing contracted:
 *   cell sums ..... photo pixel (Y, X) belongs to cell (Y h / H, X w / W) in integer arithmetic; per cell the pixel count n and the channel sums
 *                   S_c as 64-bit integers (exact); the low-resolution guide is g_c = (S_c / n) / 255, c = B, G, R.
 *   coefficients .. the window of cell (j, i) is the cells within `radius` in both axes, clipped to the grid; a window mean is the sum over it divided
 *                   by its own count, summed directly (along the row, then down the column, each in index order; no running sums). From the window
 *                   means of g (3), g g^T (6), p (the map) and g p (3): Sigma = mean(g g^T) - mean(g) mean(g)^T + eps I,
 *                   a = Sigma^-1 (mean(g p) - mean(g) mean(p)) by Cholesky, b = mean(p) - a . mean(g).
 *   their means ... the same clipped window mean of (a_B, a_G, a_R, b) -> fp64 [h, w, 4], kept in the pair's scratch and, where coeffs_f64 is not NULL,
 *                   also written there, pair p at 4 sum_{q < p} h_q w_q doubles (8-byte aligned).
 *   apply ......... per photo pixel the four mean coefficients resampled bilinearly at the pixel's centre, u = (X + 0.5) w / W - 0.5 clamped to the grid
 *                   (fp64 weights, rows first: the resampler of the tile fit and of mdpt_post_align_*), q = a_B B / 255 + a_G G / 255 + a_R R / 255 + b,
 *                   rounded to fp32 once.
 * radius 0 gives a = 0 exactly and the bilinear resize of the map; a flat photo gives the window mean of the map; a map that is an affine function of
 * the low-resolution guide comes back as that function of the photo. A value that is not finite stays inside the windows that see it.
 * Checks (MDPT_E_INVALID, nothing launched): null pointers, P outside 1 .. 65535, radius outside 0 .. 64, eps <= 0 or not finite, sizes <= 0,
 * H < h or W < w, pitch < 3 W, H W or h w >= 2^31, misaligned map / output / table / scratch / coefficients, a scratch region outside
 * scratch_bytes or overlapping another. mdpt_post_guided_scratch_bytes reads only h and w of the records: the bytes of P regions laid end to end. */
typedef struct mdpt_guided_pair { const void* map; int32_t h, w; const void* photo; int64_t pitch; int32_t H, W; void* out; int64_t scratch_off; } mdpt_guided_pair;
int mdpt_post_guided_scratch_bytes(const mdpt_guided_pair* pairs_host, int32_t P, size_t* bytes);
int mdpt_post_guided_upsample(const mdpt_guided_pair* pairs_host, const void* pairs_dev, int32_t P, int32_t map_dtype, int32_t radius, double eps,
                              void* scratch, size_t scratch_bytes, void* coeffs_f64, void* stream);

/* Rendering of depth meshes on the device (additive to ABI v6): the step of the reference's 3D viewer that needs a browser with WebGL there -
 * 3dviewer/index.html:1158-1228 render_3d with the mesh shaders of shaders.js - for the slabs mdpt_post_mesh writes, read in place with their
 * device-side counts: B meshes x V views in one call, four launches (clear, vertex stage, raster, resolve), nothing read back, nothing
 * synchronises, bit-deterministic. Inputs: xyz_f32 [B,nv,3], uv_f32 [B,nv,2], faces_i32 [B,nf,3] (MDPT_MESH_TRIANGLES) or [B,nf,1] with nf == nv
 * (MDPT_MESH_POINTS), counts_i32 [B,2] = {kept vertices, kept faces}, read on the device: vertices and faces at or beyond their image's count
 * are not read, and a face that names a vertex outside the kept ones does nothing. One uint8 BGR texture [h,w,3] per mesh: an mdpt_texture table
 * in DEVICE memory (tex_dev, 8-byte aligned; tex_host = the same records on the host, for the argument checks only). view_proj_f64 = device fp64
 * [B,V,16] in the reference's layout, row vector times matrix: clip_j = x M[j] + y M[4+j] + z M[8+j] + M[12+j] (MAT4.multiply, uniformMatrix4fv).
 *   vertex stage .. clip in fp64, nothing contracted; ndc = clip / w; screen x = (ndc_x + 1) / 2 W, y = (1 - ndc_y) / 2 H (pixel centres at + 0.5,
 *                   row 0 at the top), each snapped to 1/256 pixel: rint(256 x), int32. Kept per vertex: the snapped x, y, 1 / w and
 *                   z01 = (ndc_z + 1) / 2 in fp64. A vertex with w <= 0 or a snapped magnitude >= 2^30 is unusable and a face holding one is
 *                   dropped whole (GL clips such a face against the near plane: a stated deviation).
 *   coverage ...... int64 edge functions on the snapped coordinates at the pixel centres, top-left fill rule: a centre exactly on an edge belongs
 *                   to the face whose interior is to its right or, on a horizontal edge, below. Exact, and watertight along shared edges.
 *                   cull_back: faces that are not counter-clockwise with y up are skipped (gl.enable(CULL_FACE)); otherwise both windings draw.
 *                   Faces without area never draw.
 *   visibility .... z01 = (e0 z0 + e1 z1 + e2 z2) / (e0 + e1 + e2) in fp64 from the integer edge values e_k (opposite vertex k): linear in screen
 *                   space, as GL's depth. Fragments outside [0, 1] are discarded. key = (fp32 bits of z01) << 32 | face index, merged into a
 *                   uint64 z-buffer with a 64-bit integer atomic min: order-independent, ties go to the lower face index (LESS, drawn in order).
 *   resolve ....... per pixel, for the winning face: b_k = (e_k / w_k) / sum_j (e_j / w_j) in fp64; uv = sum b_k uv_k; the texture sampled
 *                   bilinearly as GL's LINEAR with CLAMP_TO_EDGE on level 0 (texel centres at + 0.5; v = 1 is the photo's first row), rounded to
 *                   uint8 once (floor(c + 0.5)). Mipmapped minification (LINEAR_MIPMAP_LINEAR, textures.js:200) is NOT reproduced.
 *   points ........ a square of point_size pixels centred on the snapped vertex, half = rint(128 point_size) in 1/256 pixel: the pixel centres
 *                   with x - half <= centre < x + half (y alike), carrying the vertex's uv and z01.
 * Outputs per mesh and view: color_bgra uint8 [B,V,H,W,4] (covered: alpha 255; background 0,0,0,0 = gl.clearColor(0,0,0,0)), 4-byte aligned;
 * depth_f32 [B,V,H,W] or NULL: the clip-space w (background +inf); face_id_i32 [B,V,H,W] or NULL (background -1). Limits: B V <= 65535, sides of
 * the output <= 32768, 0 < point_size <= 1024. scratch = mdpt_post_render_scratch_bytes (the z-buffer and the transformed vertices), 8-byte aligned. */
typedef struct mdpt_texture { const void* bgr; int32_t h, w; } mdpt_texture;
int mdpt_post_render_scratch_bytes(int32_t B, int32_t V, int32_t nv, int32_t nf, int32_t out_h, int32_t out_w, size_t* bytes);
int mdpt_post_render(const void* xyz_f32, const void* uv_f32, const void* faces_i32, const void* counts_i32, int32_t B, int32_t nv, int32_t nf,
                     int32_t mode, const mdpt_texture* tex_host, const void* tex_dev, const void* view_proj_f64, int32_t V, int32_t out_h, int32_t out_w,
                     int32_t cull_back, double point_size, void* color_bgra, void* depth_f32, void* face_id_i32, void* scratch, size_t scratch_bytes,
                     void* stream);

/* Hole filling of rendered views on the device (additive to ABI v6; not in the reference, whose viewer shows the holes): hierarchical (push-pull)
 * filling with a preference for the far side, for the background pixels mdpt_post_render leaves behind depth edges and outside the photo's
 * frustum. N images of one size in one call: color_bgra uint8 [N,H,W,4], depth_f32 [N,H,W] (for a rendered view the clip-space w, +inf on the
 * background). A pixel is valid iff alpha != 0 and 0 < depth < inf. Level 0 is the image, level l + 1 has ceil(h_l / 2) x ceil(w_l / 2) nodes, up
 * to the 1 x 1 level L; a node holds three colour channels and a depth as fp32, depth 0 = invalid.
 *   selection (push and pull): of up to four contributors, dmax = the largest valid depth; contributor k is kept iff it is valid and
 *                   (double)d_k >= (1.0 - band) * (double)dmax. band = 1: plain push-pull; band = 0: the farthest and its exact ties only.
 *   push l -> l + 1: node (Y, X) from the children (2Y + dy, 2X + dx) that exist, in the order (0,0) (0,1) (1,0) (1,1): no valid child -> invalid,
 *                   else every channel and the depth = the fp64 sum of the kept children in that order / their count, rounded once to fp32.
 *   pull l + 1 -> l, top down: a valid node keeps its value; an invalid node (y, x) takes Ya = y >> 1, Yb = clamp(Ya + (y odd ? 1 : -1)), x alike,
 *                   the parents (Ya,Xa) (Ya,Xb) (Yb,Xa) (Yb,Xb) with weights 9/16 3/16 3/16 1/16 (a clamped index may name a parent twice):
 *                   sum w_k v_k / sum w_k over the kept parents in fp64 in that order, rounded once: to fp32 on levels >= 1; on level 0 the
 *                   colour is floor(v + 0.5) clamped to 0 .. 255 with alpha 255 and the depth fp32. None valid: the node stays invalid.
 * Outputs (buffers of their own): out_bgra [N,H,W,4]; out_depth_f32 [N,H,W] or NULL. A pixel that was valid is copied byte for byte and bit for bit;
 * an image without a valid pixel comes out as background (0,0,0,0, depth +inf). No atomics; bit-deterministic; nothing is read back and nothing
 * synchronises; the number of launches follows from H and W alone: with t = the first level of at most 32 x 32 nodes, ceil(t / 3) push launches,
 * one launch for the levels t .. L, t pull launches (9 for 1920x1080). scratch = mdpt_post_fill_scratch_bytes (levels 1 .. L, 16 bytes per node),
 * 16-byte aligned; what it held before does not matter. Limits: N <= 65535, sides <= 32768, 0 <= band <= 1. */
int mdpt_post_fill_scratch_bytes(int32_t N, int32_t H, int32_t W, size_t* bytes);
int mdpt_post_fill_holes(const void* color_bgra, const void* depth_f32, int32_t N, int32_t H, int32_t W, double band, void* out_bgra, void* out_depth_f32,
                         void* scratch, size_t scratch_bytes, void* stream);

/* Temporally stable video depth on the device (additive to ABI v6; not in the reference, whose video demo normalises every frame on its own). The
 * relative-depth families return each map up to a scale and a shift of its own; these three stages align a clip's maps to one another, filter them
 * over time and display them with a carried range. T frames of one size per call ([T,h,w], fp32 / bf16 / fp16); a clip of any length streams through
 * in calls, the state between calls being five small device buffers that nothing reads back: the raw last frame [h,w] (the frames' dtype), the
 * last output fp32 [h,w], ab fp64 [2], the display range fp32 [2] and started int32 [2] ({chain, range}: 0 = nothing before this call).
 *   fit:     pair t: x = frame t, y = frame t - 1 (t = 0: prev_frame; started == 0: a START, no pair), over the pixels where both are finite. Round 0:
 *            w = 1; round k = 1 .. rounds: w = 1 / (1 + r^2 / (c^2 s^2)), r = a x + b - y, {a, b, s^2} of round k - 1. Each round: the weighted sums
 *            {n, Sx, Sy, Sxx, Sxy, Syy} (2048-pixel chunks, a fixed tree inside a chunk, chunks added in order), var = n Sxx - Sx^2, cov = n Sxy - Sx Sy,
 *            a = cov / var, b = (Sy - a Sx) / n, s^2 = max(0, (Syy - a Sxy - b Sy) / n). s^2 <= 2^-40 Syy / n: the frames agree exactly, the fit is kept.
 *            CUT (kept too): fewer than two samples, var <= 0, a <= 0, a result that is not finite, and for the final fit var_y <= 0 or
 *            cov^2 < cut_corr^2 var var_y. sums_f64 (or NULL) [rounds + 1, T, 6]: a kept pair repeats its last sums, a start has zeros.
 *   chain:   one lane, in order from ab_in: A_t = A_{t-1} a_t, B_t = A_{t-1} b_t + B_{t-1}, sigma_t = A_{t-1} s_t; a start, a cut, a result that is not
 *            finite or an A_t outside [2^-20, 2^20] re-anchors: A = 1, B = 0, sigma = 0, cut = 1. table_f64 [T,4] = {A, B, sigma, cut}; ab_out = the last.
 *            2 (rounds + 1) + 1 launches whatever T. prev_frame and ab_in are not read where started == 0 (they must still be valid buffers).
 *   filter:  per pixel, in frame order, o_prev from prev_out_f32 [h,w]: s = A_t p + B_t; at a cut, or where o_prev or p is not finite: o = s; else
 *            d = s - o_prev, g = d^2 / (d^2 + (tau sigma_t)^2) (0 / 0 = 0), k = alpha + (1 - alpha) g, o = o_prev + k d, and o = s where k == 1; fp64,
 *            rounded once to fp32, that fp32 being the next o_prev. out_f32 [T,h,w]. One launch; 0 < alpha <= 1, tau >= 0.
 *   display: mdpt_post_minmax_seg / _u8_hist_seg / _colorize's arithmetic (out_h = out_w = 0: no resize) with the range (lo_t, hi_t) in place of the
 *            frame's own min / max {m_t, M_t}: lo_t = fp32(lo_{t-1} + range_rate (m_t - lo_{t-1})) in fp64, hi alike; the frame's own at a cut, with
 *            started == 0, with range_rate == 1, and where one of the four is not finite; values outside the range clamp. out_bgr uint8 [T,H,W,3],
 *            ranges_f32 (or NULL) [T,2], range_out_f32 [2] = the last. Four launches. No histogram equalisation.
 * Bit-deterministic, no atomics, nothing synchronises. scratch = mdpt_post_video_scratch_bytes (covers all three for these sizes), 8-byte aligned.
 * Limits: T <= 65535, h w < 2^31, 0 <= rounds <= 8, c > 0, 0 <= cut_corr <= 1, 0 < range_rate <= 1. */
int mdpt_post_video_scratch_bytes(int32_t T, int32_t h, int32_t w, int32_t out_h, int32_t out_w, size_t* bytes);
int mdpt_post_video_fit(const void* frames, int32_t dtype, int32_t T, int32_t h, int32_t w, const void* prev_frame, const void* ab_in_f64, const void* started_i32,
                        int32_t rounds, double c, double cut_corr, void* table_f64, void* ab_out_f64, void* sums_f64, void* scratch, size_t scratch_bytes,
                        void* stream);
int mdpt_post_video_filter(const void* frames, int32_t dtype, int32_t T, int32_t h, int32_t w, const void* table_f64, const void* prev_out_f32, double alpha,
                           double tau, void* out_f32, void* stream);
int mdpt_post_video_display(const void* stable_f32, int32_t T, int32_t h, int32_t w, const void* table_f64, const void* range_in_f32, const void* started_i32,
                            int32_t out_h, int32_t out_w, int32_t reverse, const void* cmap_bgr, double range_rate, void* out_bgr, void* ranges_f32,
                            void* range_out_f32, void* scratch, size_t scratch_bytes, void* stream);

/* Synthetic depth of field on the device (additive to ABI v6; not in the reference): a photo refocused by its depth map ("portrait mode"). A focal
 * plane is put where the caller says; every photo pixel gets a blur radius from its signed defocus; the blur varies per pixel and is occlusion-aware
 * (a sharp foreground is not smeared by the blurred background behind it, a blurred foreground spreads over what is behind it). n pairs of any sizes
 * in one call, four launches whatever n is, nothing read back, nothing synchronises, no atomics, bit-deterministic, every pair independent of the
 * others. A pair is an mdpt_refocus_pair record: the h x w map (dtype), the uint8 BGR photo of H x W pixels (any size relative to the map) whose rows
 * start `pitch` bytes apart (pitch >= 3 W; no alignment is asked: the photo is read byte by byte, in place), the packed uint8 H x W x 3 output (NULL
 * in EVERY record: the preparation alone, for radius_out / defocus_out), scratch_off, the byte offset of the pair's own scratch inside `scratch` (a
 * multiple of 8; the pair needs mdpt_post_refocus_scratch_bytes of its record alone from there: 1024 bytes and 8 per photo pixel; regions must not
 * overlap), and tile_off = the sum over the pairs before it of ceil(H / 32) ceil(W / 32) (MDPT_REFOCUS_TILE = 32). The table is passed twice:
 * records_dev in DEVICE memory (8-byte aligned), records_host the same records on the host, read during the call for the argument checks only.
 * All arithmetic is fp64, nothing contracted:
 *   map ........... s(Y, X) = the map at the centre of photo pixel (Y, X): bilinear at u = (X + 0.5) w / W - 0.5 clamped to the grid, fp64 weights, rows
 *                   first (the resampler of mdpt_post_align_* and mdpt_post_guided_upsample); a map of the photo's size is read directly.
 *   defocus ....... space MDPT_ALIGN_INVERSE (relative models: the map is affine in 1 / depth): lo, hi = the fp32 min / max of the map's finite values
 *                   (a zero of either sign counts as +0), e = (s - lo) / (hi - lo) - focus, focus in [0, 1]. MDPT_ALIGN_DEPTH (metric maps):
 *                   u = 1 / s for s > 0, u = 0 for a finite s <= 0 (infinitely far), e = u - 1 / focus, focus a depth > 0. e > 0: nearer than the
 *                   focal plane. focus_xy != NULL ((x, y) in [0, 1]^2, host memory): focus is replaced by the value at photo pixel
 *                   (min(H - 1, floor(y H)), min(W - 1, floor(x W))) - (s - lo) / (hi - lo) there, or s there - read on the device, so e = 0 at it.
 *                   e = 0 where s is not finite (NaN or +-inf, in either space); e = 0 for every pixel of a pair whose map is flat or has no finite
 *                   value (inverse space), or whose pointed s is not finite or, in depth space, not > 0: that photo comes back byte for byte.
 *                   e32 = e rounded once to fp32.
 *   radius ........ r = min(max_radius, aperture max(0, |e| - focus_range / 2)) from the fp64 e; aperture = photo pixels per unit of e; quantised
 *                   to quarter pixels, rq = floor(4 r), 0 <= rq <= 4 max_radius <= 128. The footprint of a pixel is the lattice disc
 *                   {d : dx^2 + dy^2 <= k}, k = (rq rq) >> 4, its weight 1 / N(k), N(k) = the lattice points of that disc (1, 5, 9, 9, 13, ...).
 *   gather ........ for output pixel p over the taps q = p + (dy, dx) inside the photo, dy outer, dx inner, both ascending:
 *                   k_eff = k(q) if e32(q) > e32(p), else min(k(q), k(p)); where dx^2 + dy^2 <= k_eff the tap adds w B, w G, w R, w with
 *                   w = 1.0 / N(k_eff) to four fp64 sums, product then add; any other tap adds nothing. out_c = (uint8) floor(sum_c / sum_w + 0.5).
 * radius_out (or NULL): every pair's rq plane, uint8 [H, W], end to end in pair order; defocus_out (or NULL, 4-byte aligned): the e32 planes alike.
 * Checks (MDPT_E_INVALID, nothing launched, the message names the argument): null pointers, n outside 1 .. 65535, max_radius outside 0 ..
 * MDPT_REFOCUS_MAX_RADIUS, aperture or focus_range negative or not finite, focus outside its domain (without focus_xy) or focus_xy outside
 * [0, 1]^2, sizes <= 0, H W or h w >= 2^31, pitch < 3 W, a wrong tile_off, misaligned map / table / scratch, a scratch region outside scratch_bytes
 * or overlapping another, outputs in some records only. mdpt_post_refocus_scratch_bytes reads only H and W: the bytes of n regions laid end to end.
 * Known limits: what a blurred foreground edge uncovers is not inpainted; the disc is hard-edged (no bokeh shapes, no highlight boost); the average
 * is taken on the gamma-encoded bytes. */
#define MDPT_REFOCUS_MAX_RADIUS 32
#define MDPT_REFOCUS_TILE 32
typedef struct mdpt_refocus_pair { const void* map; int32_t h, w; const void* photo; int64_t pitch; int32_t H, W; void* out; int64_t scratch_off, tile_off; } mdpt_refocus_pair;
int mdpt_post_refocus_scratch_bytes(const mdpt_refocus_pair* records_host, int32_t n, int32_t max_radius, size_t* bytes);
int mdpt_post_refocus(const mdpt_refocus_pair* records_host, const void* records_dev, int32_t n, int32_t dtype, int32_t space, double focus,
                      const double* focus_xy, double aperture, double focus_range, int32_t max_radius, void* scratch, size_t scratch_bytes, void* radius_out,
                      void* defocus_out, void* stream);

/* Surface normals and relighting on the device (additive to ABI v6; not in the reference): the surface normal of every photo pixel from its depth map,
 * under the camera of mdpt_post_mesh (x right, y up, the camera looks along -z), so the normals are those of the mesh this library exports and renders;
 * as fp32 unit vectors, as an encoded uint8 normal map and / or as num_lights relit copies of the photo. n pairs of any sizes in one call, at most three
 * launches whatever n and num_lights are (inverse space: min / max, per-pair state, the tile kernel; depth space: the tile kernel alone), nothing read
 * back, nothing synchronises, no atomics, bit-deterministic, every pair independent of the others. A pair is an mdpt_normals_pair record: the h x w map
 * (dtype); the uint8 BGR photo of H x W pixels (any size relative to the map) whose rows start `pitch` bytes apart (pitch >= 3 W; read byte by byte, in
 * place; NULL in EVERY record: every photo byte is 255, a white-clay hillshade of H x W pixels); the outputs, each NULL in every record or in none -
 * normals fp32 [H,W,3] = (x, y, z), encoded uint8 [H,W,3], relit uint8 [num_lights,H,W,3] - which decide what is written; scratch_off, the byte offset of
 * the pair's own scratch inside `scratch` (a multiple of 8; 1024 bytes a pair; regions must not overlap); tile_off = the sum over the pairs before it of
 * ceil(H / 32) ceil(W / 32) (MDPT_NORMALS_TILE = 32); kx = x_scale tan(fov / 2), ky = y_scale tan(fov / 2) with (x_scale, y_scale) = (1, H / W) for
 * W > H, else (W / H, 1) (the aspect rule of mdpt_post_mesh); step = the difference step t in photo pixels, 1 .. MDPT_NORMALS_MAX_STEP. The table is
 * passed twice: records_dev in DEVICE memory (8-byte aligned), records_host the same records on the host, read during the call for the argument checks
 * only. lights_dev: fp64 [num_lights,3] UNIT directions towards the light in DEVICE memory (8-byte aligned; the caller normalises them).
 * All arithmetic is fp64, nothing contracted, every result rounded once. Per photo pixel (Y, X):
 *   sample ........ s = the map at the pixel's centre: bilinear at u = (X + 0.5) w / W - 0.5 clamped to the grid, fp64 weights, rows first (the resampler
 *                   of mdpt_post_refocus); a map of the photo's size is read directly.
 *   depth ......... space MDPT_ALIGN_INVERSE: lo, hi = the fp32 min / max of the map's finite values (a zero of either sign counts as +0),
 *                   v = hi > lo ? (s - lo) / (hi - lo) : 0, z = 1 / (a + b v), a = 1 / max_depth, b = 1 / min_depth - 1 / max_depth (mdpt_post_mesh's
 *                   non-metric depth); the pixel is valid iff s is finite. MDPT_ALIGN_DEPTH: z = s, valid iff s is finite and s > 0 (min_depth and
 *                   max_depth are not read).
 *   position ...... x = 2 (X + 0.5) / W - 1, y = 1 - 2 (Y + 0.5) / H, P = ((z x) kx, (z y) ky, -z).
 *   tangents ...... per axis, A = the neighbour at +t (x axis: X + t; y axis: Y - t, up), B the one at -t; a neighbour is usable if it lies inside the
 *                   photo and is valid. Both usable, with da = |z_A - z_0|, db = |z_0 - z_B|: da <= edge_ratio db and db <= edge_ratio da (edge_ratio =
 *                   inf: always, the products are not formed) -> T = P_A - P_B; else T = P_A - P_0 if da < db, else P_0 - P_B. One usable: that
 *                   side. None usable on either axis, or the centre invalid: the pixel is invalid. A normal is never taken across a depth edge.
 *   normal ........ n = Tx x Ty = (Tx.y Ty.z - Tx.z Ty.y, Tx.z Ty.x - Tx.x Ty.z, Tx.x Ty.y - Tx.y Ty.x), len2 = (nx nx + ny ny) + nz nz; invalid unless
 *                   len2 is finite and > 0; n_c / sqrt(len2). No flip: a height field seen from the origin faces the camera. An invalid pixel gets
 *                   (0, 0, 0). normals = fp32(n). encoded byte = floor((c + 1) / 2 * 255 + 0.5) of the fp64 component, stored B, G, R = z, y, x
 *                   (invalid: 128, 128, 128).
 *   shading ....... per light l: d = n.l = (nx lx + ny ly) + nz lz, shade = ambient + diffuse (d > 0 ? d : 0). specular > 0: view_c = -P_c / |P|,
 *                   |P| = sqrt((Px Px + Py Py) + Pz Pz), h_c = (l_c + view_c) / |l + view| alike, sp = n.h (> 0, else 0; the sum formed as for d),
 *                   squared shininess_log2 times (repeated squaring, no pow), spec = 255 (specular sp); else spec = 0.
 *                   relit_c = min(255, floor((photo_c shade + spec) + 0.5)). An invalid pixel returns the photo's bytes. The mix is on the
 *                   gamma-encoded bytes of a photo that carries its own lighting; no cast shadows, no ambient occlusion.
 * Checks (MDPT_E_INVALID, nothing launched, the message names the argument): null pointers, n outside 1 .. 65535, num_lights outside 0 ..
 * MDPT_NORMALS_MAX_LIGHTS, relit outputs without lights, min_depth / max_depth outside 0 < min < max < inf (inverse space), edge_ratio < 1 or NaN,
 * ambient / diffuse / specular negative or not finite, shininess_log2 outside 0 .. 10, sizes <= 0, H W or h w >= 2^31, pitch < 3 W, step outside its
 * range, kx / ky not finite or <= 0, a wrong tile_off, misaligned map / table / lights / scratch / normals, a scratch region outside scratch_bytes or
 * overlapping another, an output or the photo in some records only, no output at all. mdpt_post_normals_scratch_bytes reads only H and W. */
#define MDPT_NORMALS_MAX_STEP 16
#define MDPT_NORMALS_TILE 32
#define MDPT_NORMALS_MAX_LIGHTS 64
typedef struct mdpt_normals_pair { const void* map; int32_t h, w; const void* photo; int64_t pitch; int32_t H, W; void* normals; void* encoded; void* relit; int64_t scratch_off, tile_off; double kx, ky; int32_t step, pad; } mdpt_normals_pair;
int mdpt_post_normals_scratch_bytes(const mdpt_normals_pair* records_host, int32_t n, size_t* bytes);
int mdpt_post_normals(const mdpt_normals_pair* records_host, const void* records_dev, int32_t n, int32_t dtype, int32_t space, double min_depth,
                      double max_depth, double edge_ratio, const void* lights_dev, int32_t num_lights, double ambient, double diffuse, double specular,
                      int32_t shininess_log2, void* scratch, size_t scratch_bytes, void* stream);

/* Cast shadows and ambient occlusion for the relighting, on the device (additive to ABI v6; not in the reference): screen-space shadow marches and
 * horizon occlusion on a small working grid of gh x gw nodes per pair, resized to the photo and folded into the shading of mdpt_post_normals. n pairs of
 * any sizes in one call, at most four launches whatever n and num_lights are (inverse space: min / max, per-pair state; the grid kernel; the shade
 * kernel), nothing read back, nothing synchronises, no atomics, bit-deterministic, every pair independent of the others. A pair is an mdpt_shadows_pair
 * record: map, h, w, photo, pitch, H, W, scratch_off (1024 bytes a pair), tile_off, kx, ky (the PHOTO's) and step as in mdpt_normals_pair; gh, gw = the
 * working grid (any positive size, gh gw < 2^31; node (i, j) is pixel (i, j) of a gh x gw image over the photo's field of view); gtile_off = the sum over
 * the pairs before it of ceil(gh / 32) ceil(gw / 32); and three outputs, each NULL in every record or in none: ao fp32 [gh,gw], vis fp32
 * [num_lights,gh,gw] (4-byte aligned), relit uint8 [num_lights,H,W,3]. With relit the planes are the call's working memory as well: vis is required
 * where shadow_reach > 0, ao where ao_reach > 0 and ao_strength > 0; without relit the call computes the planes alone. lights_dev as for
 * mdpt_post_normals. All arithmetic is fp64, nothing contracted, only + - * / sqrt floor and comparisons, every stored value rounded once.
 * Per grid node (i, j):
 *   depth ......... s = the map at the node's centre (the sample rule of mdpt_post_normals with H, W := gh, gw; a map of the grid's size is read
 *                   directly), z by its depth rule (lo, hi are the map's), x0 = 2 (j + 0.5) / gw - 1, y0 = 1 - 2 (i + 0.5) / gh,
 *                   P = ((z x0) kx, (z y0) ky, -z). n = the normal of mdpt_post_normals on the grid at a step of one node with edge_ratio. A node
 *                   without z or without n has ao = 1 and vis = 1 for every light.
 *   occlusion ..... the eight directions (di, dj) = (0,1) (-1,1) (-1,0) (-1,-1) (0,-1) (1,-1) (1,0) (1,1) in this order; for k = 1 .. ao_reach:
 *                   q = (i + k di, j + k dj); off the grid ends the direction, an invalid q is skipped; D = P_q - P_0, l2 = (Dx Dx + Dy Dy) + Dz Dz,
 *                   hgt = ((Dx nx + Dy ny) + Dz nz) / sqrt(l2), fall = 1 - l2 / (rad rad) with rad = ao_radius z_0, rise = hgt - ao_bias,
 *                   term = (rise > 0 ? rise : 0) (fall > 0 ? fall : 0); occ_d = the largest term (a term that is not > the running maximum, which
 *                   starts at 0, is dropped). sum = (((0 + occ_0) + occ_1) + ...) + occ_7, open = 1 - (ao_strength sum) / 8,
 *                   ao = fp32(open > 0 ? open : 0).
 *   shadow ........ per light L: gx = (Lx / kx + x0 Lz) gw, gy = -((Ly / ky + y0 Lz) gh), the projected direction of the ray P_0 + t L. Both zero, or
 *                   either not finite: lit. Else the major axis c is x if |gx| >= |gy|, else y; m = |g_c|, sx = gx / m, sy = gy / m. For
 *                   k = 1 .. shadow_reach: q = (i + floor(k sy + 0.5), j + floor(k sx + 0.5)); off the grid: lit, the march ends. cq = x or y of q
 *                   (formed as x0 / y0 are), t = ((z_0 k_c) (cq - c_0)) / (L_c + (Lz k_c) cq), zr = z_0 - t Lz; t not > 0 or zr not > 0: lit, ends.
 *                   q occludes iff z_q is valid and z_q < zr (1 - shadow_bias) and (shadow_thickness = inf or zr - z_q <= shadow_thickness zr); the
 *                   first occluder sets vis = 0 and ends the march. vis is 0 or 1.
 * Per photo pixel (Y, X): the normal, d, sp, the photo bytes and the invalid pixels of mdpt_post_normals, with a = the ao plane and s_v = light v's vis
 * plane at the pixel's centre (the sample rule again, fp32 planes of gh x gw under an H x W photo; the constant 1 where the factor is off, no plane
 * read): shade = ambient a + (diffuse (d > 0 ? d : 0)) s_v, spec = 255 ((specular sp) s_v), relit_c = min(255, floor((photo_c shade + spec) + 0.5)).
 * With shadow_reach = 0 and ao_strength = 0 (or ao_reach = 0) every byte equals mdpt_post_normals'.
 * Checks (MDPT_E_INVALID, nothing launched): those of mdpt_post_normals on the shared arguments, and shadow_reach / ao_reach outside 0 ..
 * MDPT_SHADOWS_MAX_REACH, shadow_bias outside [0, 1), shadow_thickness negative or NaN, ao_radius not finite or <= 0, ao_bias or ao_strength negative
 * or not finite, a bad grid size, a wrong gtile_off, misaligned planes, a plane in some records only, a plane the shading needs missing, vis or relit
 * without lights, no output at all. Known limits: screen space only - what lies outside the frame or behind the first surface casts nothing; the
 * thickness of an occluder is assumed; a march reaches at most 32 grid nodes; the bilinear resize of the planes is the only penumbra; the mix is on
 * the gamma-encoded bytes. */
#define MDPT_SHADOWS_MAX_REACH 32
#define MDPT_SHADOWS_AO_DIRECTIONS 8
typedef struct mdpt_shadows_pair { const void* map; int32_t h, w; const void* photo; int64_t pitch; int32_t H, W, gh, gw; void* ao; void* vis; void* relit; int64_t scratch_off, tile_off, gtile_off; double kx, ky; int32_t step, pad; } mdpt_shadows_pair;
int mdpt_post_shadows_scratch_bytes(const mdpt_shadows_pair* records_host, int32_t n, size_t* bytes);
int mdpt_post_shadows(const mdpt_shadows_pair* records_host, const void* records_dev, int32_t n, int32_t dtype, int32_t space, double min_depth,
                      double max_depth, double edge_ratio, const void* lights_dev, int32_t num_lights, double ambient, double diffuse, double specular,
                      int32_t shininess_log2, int32_t shadow_reach, double shadow_bias, double shadow_thickness, int32_t ao_reach, double ao_radius,
                      double ao_bias, double ao_strength, void* scratch, size_t scratch_bytes, void* stream);

/* Depth segmentation on the device (additive to ABI v6; not in the reference): the depth-connected surfaces of a map as a label plane, a table of
 * the regions, and "the region under this point" as a mask and a BGRA cutout of the photo. The entry points are named mdpt_segment_*, not
 * mdpt_post_*: the table of the mdpt_post_* entry points and their refusals is recorded (tests/post_refusal_cases.py and its golden file), and these
 * have a record of their own (tests/test_segment_cpu.py). Any number of images per call, each independent of the others.
 * An image is an mdpt_segment_image record: the h x w map (dtype), its int32 [h,w] label output, scratch_off (bytes from `scratch`, a multiple of 8; the
 * image needs mdpt_segment_scratch_bytes of its record alone from there; regions must not overlap), region_off = the rows of the region tables of
 * the images before it (image i has R_i = (h w) / min_area rows, an exact bound), tile_off = the sum over the images before it of ceil(h / 32)
 * ceil(w / 32) (MDPT_SEGMENT_TILE = 32) and pixel_off = the sum of their h w. The table is passed twice: records_host (read by the checks) and
 * records_dev, its copy in device memory, 8-byte aligned (read by the kernels).
 *   validity ...... a node is valid iff its value v (widened to fp32) is finite and, in space MDPT_ALIGN_DEPTH, v > 0. lo, hi = the min / max of the
 *                   image's valid nodes as fp64 (a zero takes the sign +; no valid node: 0, 0) -> range[2 i], range[2 i + 1].
 *   links ......... two valid neighbours p, q are linked iff, in fp64 on the exact fp32 values, |v_p - v_q| <= step (hi - lo) (MDPT_ALIGN_INVERSE)
 *                   or <= step min(v_p, v_q) (MDPT_ALIGN_DEPTH); neighbours: the 4 along the axes (connectivity 4) or those and the 4 diagonals (8).
 *   components .... the connected sets of valid nodes under the links; a component's root is its lowest linear index y w + x. Components of fewer
 *                   than min_area nodes are dropped; the K kept ones are numbered 0 .. K - 1 in the order of their roots -> counts[i] = K.
 *   labels ........ a node's region, -1 for a node that is not valid or whose component was dropped.
 *   per region .... (row region_off + r) area int32; bbox int32 x 4 = x0, y0, x1, y1 inclusive; first int32 = the root; vrange fp32 x 2 = the least and
 *                   the greatest value; sum_q int64 = the sum of floor((v - lo) / (hi - lo) 2^24 + 0.5) in fp64 (0 where hi == lo).
 * Ten launches whatever n is: min / max partials, state, a union-find per 32 x 32 tile in LDS, a lock-free merge of the pairs across tile edges
 * (atomic min, larger root under smaller), flatten + areas, flags, scan, scatter, relabel + statistics, finish. Integer atomics only, every output
 * bit-deterministic, nothing read back, no synchronisation.
 * mdpt_segment_colors: labels -> uint8 BGR [h w, 3] per image at colors + 3 pixel_off, a fixed integer hash of the label, -1 black. One launch.
 * mdpt_segment_cutout: a photo is an mdpt_segment_photo record - the int32 [h,w] labels, the uint8 BGR photo of H x W pixels whose rows lie `pitch`
 * bytes apart, its BGRA [H,W,4] (4-byte aligned) and mask [H,W] outputs, region_off as above and regions = R_i. picks_dev = int32 [num_picks, 2] in
 * device memory, {image, value}: value is a node's linear index (by_label = 0: the region under it is selected; a -1 node selects nothing) or a
 * region (by_label != 0); anything out of range selects nothing. selected = uint8, one per region row of the call, ZERO on entry, marked by the
 * first launch. Photo pixel (Y, X) belongs to node ((Y h) / H, (X w) / W), integer division; mask = 255 where that node's region is selected,
 * flipped by invert; BGRA = (BGR AND mask, mask). Two launches (one without picks) whatever n is.
 * Checks (MDPT_E_INVALID, nothing launched, the message names the argument): null pointers, n outside 1 .. 65535, sizes <= 0 or h w >= 2^31, step
 * negative or not finite, connectivity not 4 or 8, min_area < 1, a bad dtype or space, wrong region_off / tile_off / pixel_off, misaligned pointers,
 * a photo pitch < 3 W, num_picks < 0 or picks without picks_dev, a scratch region or `selected` too small, misaligned or overlapping.
 * Known limits: a surface at a grazing angle has large steps between neighbours and breaks into slivers; a gentle ramp (the ground) connects what
 * stands on it to the background; regions below min_area are dropped, not merged into a neighbour. */
#define MDPT_SEGMENT_TILE 32
typedef struct mdpt_segment_image { const void* map; int32_t h, w; void* labels; int64_t scratch_off, region_off, tile_off, pixel_off; } mdpt_segment_image;
typedef struct mdpt_segment_photo { const void* labels; int32_t h, w; const void* photo; int64_t pitch; int32_t H, W; void* bgra; void* mask; int64_t region_off; int32_t regions, pad; } mdpt_segment_photo;
int mdpt_segment_scratch_bytes(const mdpt_segment_image* records_host, int32_t n, size_t* bytes);
int mdpt_segment_depth(const mdpt_segment_image* records_host, const void* records_dev, int32_t n, int32_t dtype, int32_t space, double step,
                       int32_t connectivity, int32_t min_area, void* scratch, size_t scratch_bytes, void* counts, void* area, void* bbox, void* first,
                       void* vrange, void* sum_q, void* range, void* stream);
int mdpt_segment_colors(const mdpt_segment_image* records_host, const void* records_dev, int32_t n, void* colors, void* stream);
int mdpt_segment_cutout(const mdpt_segment_photo* records_host, const void* records_dev, int32_t n, const void* picks_dev, int32_t num_picks,
                        int32_t by_label, void* selected, size_t selected_bytes, int32_t invert, void* stream);

/* Locally varying true-depth alignment on the device (additive to ABI v6; not in the reference): depth completion from a relative-depth map and a
 * measured depth map that is partly valid and at its own resolution (a LiDAR sweep, a structure-from-motion point set, a cheap sensor). Where
 * mdpt_post_align_* fit one (A, B) per image, these fit one per cell of a grid over the truth, smooth them, and apply the coefficient FIELD, so that a
 * drift of the prediction's error across the frame does not stay in the result. Named mdpt_localfit_*, not mdpt_post_*, for the reason
 * mdpt_segment_* are (the recorded table of the mdpt_post_* entry points); their record is tests/test_local_align_cpu.py. Any number of pairs per
 * call, each independent of the others, sizes and grids may all differ.
 * A pair is an mdpt_localfit_pair record: the seven fields of an mdpt_depth_pair record - pred ph x pw of pred_dtype, truth fp32 H x W, valid uint8 H x W or
 * NULL - the grid gh x gw (1 <= gh <= H, 1 <= gw <= W, both <= MDPT_LOCALFIT_MAX_GRID = 256), cell_off = the sum of gh gw over the pairs before it
 * (its rows of the moment and coefficient tables), scratch_off (bytes from `scratch`, a multiple of 8; the pair needs mdpt_localfit_scratch_bytes
 * of its record alone from there; regions must not overlap) and out (apply only). The table is passed twice: records_host (read by the checks) and
 * records_dev, its copy in device memory, 8-byte aligned (read by the kernels). All arithmetic fp64, nothing contracted, results rounded once.
 *   samples ....... exactly those of mdpt_post_align_fit with MDPT_ALIGN_LSTSQ: the same validity rule and truth range [tmin, tmax], v = the
 *                   prediction at the centre of the truth pixel by the same resampler, t = 1 / truth (MDPT_ALIGN_INVERSE) or truth (MDPT_ALIGN_DEPTH).
 *   cell moments .. the sample at truth pixel (Y, X) belongs to cell (Y gh / H, X gw / W), integer division (mdpt_post_guided_upsample's rule). Per
 *                   cell M = {n, Sv, St, Svv, Svt, Stt} -> moments_f64 [cells of the call, 6]. A cell's pixels are taken in row-major order inside
 *                   the cell, in chunks of MDPT_LOCALFIT_CHUNK = 2048: a workgroup reduces one chunk (thread t its pixels t, t + 256, ... in order,
 *                   then a fixed tree) and the next launch adds a cell's chunks in chunk order. The split depends on the pair's own H, W, gh, gw only.
 *   global fit .... G = the cells' M added in row-major cell order -> sums_f64 [P, 6]; (A0, B0) from G by mdpt_post_align_fit's solve rule, its
 *                   degenerate rule included -> fit_f64 [P, 2].
 *   window fit .... node (j, i): the M of the cells with |dj| <= radius and |di| <= radius, clipped to the grid, one running sum with dj outer and di
 *                   inner, both ascending. A window without a sample takes (A0, B0). Otherwise, where prior > 0 and n_G > 0, prior (G_k / n_G) is
 *                   added term by term (prior pseudo-samples distributed as the image's own), and the sums are solved by the same rule; a degenerate
 *                   window (n < 2, var <= 0, A not finite or <= 0) takes (A0, B0). prior = 0: the pure local fit; prior large: the global fit.
 *   coefficients .. C[j, i] = the window fits summed over the same clipped window in the same order, divided by its cell count (the guided
 *                   filter's second averaging) -> coeffs_f64 [cells of the call, 2].
 *   apply ......... per pixel (Y, X) of the record's H x W (the OUTPUT size here; truth and valid are not read and may be NULL; the grid need not fit
 *                   inside it) (A, B) = C resampled at the pixel's centre, u = (X + 0.5) gw / W - 0.5 clamped to the grid, fp64 weights, rows first,
 *                   A and B separately; v = the prediction at the pixel's centre; q = A v + B; from there as mdpt_post_align_apply: 1 / q with +inf
 *                   where q <= 0 in inverse space, q in depth space, clamped to [dmin, dmax] where finite, rounded to fp32 once -> out. NaN stays NaN.
 * mdpt_localfit_fit: FIVE launches whatever n is (chunk partials, cells, global fit, window fits, coefficient means); mdpt_localfit_apply: ONE. No
 * atomics, nothing read back, no synchronisation, bit-deterministic. The window sums are direct: (2 radius + 1)^2 additions a node.
 * Checks (MDPT_E_INVALID, nothing launched, the message names the argument): null pointers, n outside 1 .. 65535, sizes <= 0 or H W >= 2^31, a grid
 * larger than the truth or over the cap, radius outside 0 .. MDPT_LOCALFIT_MAX_RADIUS = 64, prior negative or not finite, tmin > tmax, dmin > dmax,
 * a bad dtype or space, a wrong cell_off, misaligned pointers, a scratch region outside the scratch, misaligned or overlapping.
 * Not done here: edge-aware (photo-guided) propagation of the coefficients, robust reweighting of outliers, a median variant, per-node confidence,
 * temporal coherence. */
#define MDPT_LOCALFIT_MAX_GRID 256
#define MDPT_LOCALFIT_MAX_RADIUS 64
#define MDPT_LOCALFIT_CHUNK 2048
typedef struct mdpt_localfit_pair { const void* pred; int32_t ph, pw; const void* truth; const void* valid; int32_t H, W, gh, gw; int64_t cell_off, scratch_off; void* out; } mdpt_localfit_pair;
int mdpt_localfit_scratch_bytes(const mdpt_localfit_pair* records_host, int32_t n, size_t* bytes);
int mdpt_localfit_fit(const mdpt_localfit_pair* records_host, const void* records_dev, int32_t n, int32_t pred_dtype, int32_t space, int32_t radius,
                      double prior, double tmin, double tmax, void* moments_f64, void* fit_f64, void* sums_f64, void* coeffs_f64, void* scratch,
                      size_t scratch_bytes, void* stream);
int mdpt_localfit_apply(const mdpt_localfit_pair* records_host, const void* records_dev, int32_t n, int32_t pred_dtype, int32_t space,
                        const void* coeffs_f64, double dmin, double dmax, void* stream);

/* Stage boundaries of the LAST mdpt_forward on `workspace`, converted to reference layouts (debug / parity taps):
 * which = 0..3 encoder taps [B,N,F]; 4..7 reassembly maps (BCHW); 8 fused map [B,C,8gh,8gw]. */
int mdpt_export_tap(mdpt_handle* h, int32_t which, void* out_f32, void* workspace, size_t workspace_bytes, void* stream);

/* Test hooks (used by tests/ only): stop the encoder of the next mdpt_forward calls after sub-step `step` of transformer
 * block `block` (0 LN1, 1 QKV, 2 attention, 3 proj+residual, 4 LN2, 5 fc1+GELU, 6 fc2+residual; block = -1 disables), and
 * read an internal activation buffer ("resid","xn","q","k","vt","att","hbuf","im2col","pos","t0".."t3","u0","u1","d3",
 * "xf0".."xf3","a10".."a13","b20".."b23","flo0".."flo3","fused","h1","h1u") of the last forward as flat fp32 in its internal layout. */
int mdpt_debug_set_stop(mdpt_handle* h, int32_t block, int32_t step);
/* Test hook: latency mode's K split of the residual GEMMs applies from `min_k_tiles` 64-wide K tiles on (two ranges) and from
 * `four_k_tiles` on as four ranges (toy models have 4 K tiles). */
int mdpt_debug_set_ksplit_min(mdpt_handle* h, int32_t min_k_tiles, int32_t four_k_tiles);
/* Test / A-B hook: unsplit forwards (batches below mdpt_set_batch_split's threshold, i.e. the reference's frame-by-frame workload) queue each
 * reassembly branch (reassembly_model.py:61-94: four independent branches, one per encoder tap) on the handle's internal side stream as soon
 * as its tap exists, beside the remaining encoder blocks, and join before the fusion stage - same kernels, same bits, stream-ordering
 * semantics for the caller unchanged (as for the batch split). `on`: 0 = never (branches behind the encoder on the caller's stream), 1 = the
 * library's rule (default: encoders of width >= 1024 outside latency mode, where it measured faster), 2 = always. */
int mdpt_debug_set_reassemble_overlap(mdpt_handle* h, int32_t on);
/* Test / A-B hooks of the internal side stream, to be set before the first forward creates it. The runtime multiplexes the streams of a process
 * onto a few hardware queues; a side stream on the caller's queue would run the two halves of a split batch one after the other, so the first
 * forward on a caller stream PROBES up to four candidate streams on the GPU and keeps one that really runs beside the caller's (one host wait,
 * once per handle and caller stream, never inside a stream capture; csrc/stream_probe.hip). `probe` 0 takes the first candidate unseen.
 * Caveats of the probe: its host wait would invalidate a GLOBAL-mode stream capture another thread has open at that moment (run one forward before
 * capturing, or switch the probe off); a probe in which every candidate was rejected (GPU busy with other work) is repeated by the next forward, three
 * times at most; a stream handle recycled by the runtime after hipStreamDestroy keeps the pick of its predecessor.
 * `prio`: priority class of the candidates, 0 = default class (default), 1 = the device's lowest, -1 = highest (own queue pool, but measured
 * slower: the two classes do not overlap). mdpt_debug_side_stream_info: candidates created / candidates found on the caller's queue so far. */
int mdpt_debug_set_wscale_policy(mdpt_handle* h, int32_t all);  /* 1: scale every layer-scale-folded matrix of the fp16 build (the other valid rounding) */
int mdpt_debug_set_side_stream_priority(mdpt_handle* h, int32_t prio);
int mdpt_debug_set_side_stream_probe(mdpt_handle* h, int32_t on);
int mdpt_debug_side_stream_info(mdpt_handle* h, int32_t* candidates, int32_t* rejected);
int mdpt_debug_read(mdpt_handle* h, const char* name, void* out_f32, size_t out_floats, void* workspace, size_t workspace_bytes,
                    void* stream);

/* The handle-less kernel hooks below (mdpt_debug_gemm / _attention / _conv3 / _gemm_form / _ksplit_finish / _attention_form / _attn_weights_form) take their 16-bit operands as bf16 (0, default) or fp16 (1):
 * process-wide switch, tests only. */
int mdpt_debug_set_operand_format(int32_t fp16);

/* Kernel micro-benchmark hook: `iters` launches of the dense GEMM kernel, out[M,N] = A[M,K] * W[N,K]^T (bf16 operands,
 * fp32 and/or bf16 output), tile as in mdpt_set_gemm_tile. */
int mdpt_debug_gemm(const void* a_bf16, const void* w_bf16, void* out_f32, void* out_bf16, int32_t M, int32_t N, int32_t K,
                    int32_t tile, int32_t iters, void* stream, void* dbg_times_or_null);
/* test/bench hook: the fused attention kernel (replaces F.scaled_dot_product_attention, v2_depthanything/components/transformer_block.py:164)
 * on caller-provided head-major bf16 operands: Q (pre-scaled by 1/sqrt(64)), K [B, heads, npad, 64]; Vt [B, heads, 64, npadv] with zero pad
 * columns; out [B * npad, heads * 64]. */
int mdpt_debug_attention(const void* q_bf16, const void* k_bf16, const void* vt_bf16, void* out_bf16, int32_t B, int32_t heads, int32_t N,
                         int32_t npad, int32_t npadv, int32_t iters, void* stream);
/* test hook: ONE launch of the fused attention in any of its forms on caller-provided device buffers. The record mirrors the launcher's internal
 * parameter block field for field (csrc/mdpt_kernels.h AttnParams has the meaning of each; tail_last, which the launcher sets itself, is left
 * out): 16-bit planes in the format of mdpt_debug_set_operand_format, null = absent. x3: the three-pass form on hi + lo planes. bias_lut / tq / tk:
 * the additive table, s[q][k] += lut[h][tq[q] - tk[k]]. rowmap != null: SwinV2 window attention (head_dim 32, B = images * win_nw, region ids or null,
 * bias_run4 / bias_row / bias_ww, swin_ls, out_ld). allow_split_kv: the latency form where the launcher's rule takes it. Nothing is allocated; sizes
 * are the caller's. The launcher's own argument checks apply: a combination it refuses returns a positive HIP error code and launches nothing. */
typedef struct mdpt_attn_form {
    const void* q_hi; const void* q_lo; const void* k_hi; const void* k_lo;
    const void* vt_hi; const void* vt_lo;
    void* out_hi; void* out_lo;
    int32_t B, heads, N, npad, npadv, F;
    int32_t x3;
    const float* bias_lut; int32_t bias_elen; const int32_t* tq; const int32_t* tk;
    int32_t head_dim;
    int32_t win_nw; const int32_t* rowmap; const int32_t* region; int32_t region_ld;
    int32_t bias_run4;
    int32_t bias_row;
    int32_t bias_ww;
    const float* swin_ls;
    int32_t out_ld;
    int32_t allow_split_kv;
} mdpt_attn_form;
int mdpt_debug_attention_form(const mdpt_attn_form* form, void* stream);
/* ... and the diagnostic weights dump of the same record: out_f32 [B, heads, N, N] = the softmax probabilities (natural units) */
int mdpt_debug_attn_weights_form(const mdpt_attn_form* form, void* out_f32, void* stream);
/* test/bench hook: one 3x3 stride-1 conv Cin -> Cout (256 = the decoder's fusion width, every epilogue form; 128 = the head's first conv,
 * bias only) on caller-provided operands, through the implicit-GEMM
 * kernels (path 0, tile = MDPT_TILE_*) or the halo-staged kernel (path 1). Replaces one nn.Conv2d(…, 3, padding=1) of the reference's
 * ResidualConv2D / fusion blocks (v2_depthanything/fusion_model.py:178-182,210-220) incl. its skip add and the x2-upsampled prior. */
int mdpt_debug_conv3(const void* in_bf16, const void* w_packed_bf16, const void* bias_f32, const void* skip_f32, const void* up_f32, int32_t Hu,
                     int32_t Wu, void* out_f32, void* out_bf16, int32_t relu_bf16, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                     int32_t path, int32_t tile, int32_t iters, void* stream, void* dbg_times, const void* in_lo_bf16_or_null,
                     const void* w_lo_bf16_or_null, void* out_lo_bf16_or_null);  /* lo planes: the bf16x3 (fp32-class) mode */
/* test hook: ONE launch of the GEMM family in any of its operand / epilogue forms on caller-provided device buffers. The record mirrors the
 * launcher's internal parameter block field for field (csrc/mdpt_kernels.h GemmParams has the meaning of each; the fp8 fields and the SwinV2
 * QKV epilogue are left out): 16-bit operand and output planes in the format of mdpt_debug_set_operand_format, fp32 everything else, null =
 * absent. amode: 0 dense rows, 1 token rows (tok_*), 2 3x3 taps over NHWC (Hi .. cstride; the hook supplies the zero page). ekind: 0 generic
 * (bias .. wscale, out_*), 1 QKV (q_hi .. qscale), 2 patch + pos (pos, tok_np, npad, out_f32), 3 depth-to-space (d2s_*, Ho, Wo, out_hi / out_lo),
 * 4 depth head (head_*; N = 32). tile: 0 = the launcher's rule, 1 128x128, 2 256x256, 4 256x128, 5 8-phase 256x256, 6 64x64. ksplit > 1: K in
 * ranges, partial planes at ks_part (ks_all: every range). Nothing is allocated besides the hook's own 256-byte zero page; sizes are the caller's.
 * The launcher's own argument checks apply: a combination it refuses returns a positive HIP error code and launches nothing. */
typedef struct mdpt_gemm_form {
    const void* a_hi; const void* a_lo; const void* w_hi; const void* w_lo;
    int32_t M, N, K, lda, ldw, npass;
    int32_t amode, ekind, tile, act;
    int32_t tok_np, tok_stride;
    int32_t Hi, Wi, Cin, Ho, Wo, cstride;
    const void* bias; const void* gamma; const void* resid;
    int32_t ldr, bias_img_stride, bias_img_rows;
    void* out_f32; void* out_hi; void* out_lo;
    int32_t ldc, relu_bf16, acc_init;
    const void* wscale;
    void* q_hi; void* q_lo; void* k_hi; void* k_lo; void* vt_hi; void* vt_lo;
    int32_t F, heads, npad, npadv;
    float qscale;
    const void* pos;
    int32_t d2s_k, d2s_cout;
    const void* head_w; const void* head_b; void* head_out;
    int32_t head_sigmoid, head_out_dtype;
    int32_t ksplit, ks_all;
    void* ks_part;
} mdpt_gemm_form;
int mdpt_debug_gemm_form(const mdpt_gemm_form* form, void* stream);
/* ... and the finishing kernel behind a ks_all launch of the same record: out_f32 / out_hi / out_lo [M, N] (row stride ldc) = the sum of the ksplit
 * partial planes at ks_part in the order z = 0, 1, ... (+ bias); relu_bf16 applies a ReLU to the operand planes only. */
int mdpt_debug_ksplit_finish(const mdpt_gemm_form* form, void* stream);

/* Per-launch HIP-event profiler (bench.py's roofline leg): events are recorded on the launch stream around every
 * kernel launch while enabled. mdpt_profile_report() waits for the recorded events and writes a JSON summary
 * {"kernels":[{"name","launches","total_ms","avg_us","gflop","tflops"}...]} (algorithmic flops: 2*M*N*K per GEMM). */
int mdpt_profile_enable(int on);
int mdpt_profile_report(char* json_buf, size_t capacity);

/* Tuning knob for benchmarks: force a GEMM tile (0 = auto, 1 = 128x128, 2 = 256x256). */
int mdpt_set_gemm_tile(mdpt_handle* h, int32_t tile);

/* Data-parallel output collective (north star: "RCCL all-gather of the output depth maps"): thin wrapper over
 * ncclAllGather on a communicator created by the caller (torch.distributed's RCCL comm is used in the binding, so
 * this entry point is for non-torch hosts). `comm` is an ncclComm_t, `dtype` the element type of the maps (MDPT_DTYPE_*: the depth
 * maps travel in the dtype mdpt_forward wrote them in). Loaded lazily from librccl.so. */
int mdpt_allgather(void* comm, const void* send_dev, void* recv_dev, size_t count_per_rank, int32_t dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDPT_H */
