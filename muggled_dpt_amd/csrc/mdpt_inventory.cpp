// libmdpt: parameter inventory (reference "new format" key names), packed-weight layout and activation workspace plan.
#include "mdpt_internal.h"

namespace mdpt {

thread_local std::string g_err = "";
int g_debug_f16 = 0;

int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

const char* const kStageNames[4] = {"spatial_upx4", "spatial_upx2", "spatial_noscale", "spatial_downx2"};
const char* const kSwinStageNames[4] = {"spatial_noscale", "spatial_downx2", "spatial_downx4", "spatial_downx8"};

static std::string blk_name(const mdpt_handle* h, int block) {
    char buf[96];
    if (h->cfg.family == MDPT_FAMILY_DAV1) snprintf(buf, sizeof(buf), "imgencoder.blocks.%d", block);
    else snprintf(buf, sizeof(buf), "imgencoder.stages.%d.blocks.%d", block / h->bps, block % h->bps);
    return buf;
}
// reference attribute names differ between the families (v2: fusion_model.py:100,138 / v31_beit, v31_swinv2 fusion_model.py)
static const char* rcu_seq(const mdpt_handle* h) { return is_midas(h) ? "conv_seq" : "resconv_seq"; }
static const char* proj_seq(const mdpt_handle* h) { return is_midas(h) ? "proj_seq" : "scale_proj_seq"; }

// which classes CAN run their cross terms on fp8 planes (MDPT_PASSES_2F8 / _3F8, f8_cross.h): fp16 operands, every contraction length of
// the class a multiple of the 128-element fp8 K tile, ViT / BEiT encoders (the SwinV2 tap producers write 16-bit planes only). A class that
// cannot runs the fp16-plane form of the same term count. A property of the configuration: never of the batch or the image size.
void compute_f8ok(mdpt_handle* h) {
    for (int i = 0; i < NCLS; ++i) h->f8ok[i] = false;
    const bool base = h->f16 && !h->swin;
    const bool cp = base && h->Cp % 128 == 0;
    bool re = base && h->F % 128 == 0;
    for (int i = 0; i < 4; ++i) re = re && h->hidp[i] % 128 == 0;
    h->f8ok[CLS_REASM] = re;
    h->f8ok[CLS_FUSION] = h->f8ok[CLS_FUSION_IN] = h->f8ok[CLS_FUSION_PROJ] = h->f8ok[CLS_HEAD] = cp;
}

static void build_inventory_swin_encoder(mdpt_handle* h);
static void build_inventory_decoder(mdpt_handle* h);
static int check_weight_refs(const mdpt_handle* h);

// The one place a parameter is spelled: every add_spec names it (mdpt_weight_name order), every add_mat / add_vec states what is packed from
// which spec, in which op class and pack-time form, and the reference it returns goes into h->w for the stage drivers.
int build_inventory(mdpt_handle* h) {
    const int F = h->F, P = h->P;
    const int G = h->cfg.base_patch_grid_h * h->cfg.base_patch_grid_w;
    h->specs.clear(); h->spec_index.clear(); h->mats.clear(); h->vecs.clear();
    h->w = WeightRefs();
    WeightRefs& w = h->w;
    h->packed_total = 0;
    h->wrc_maxn = h->wrc_maxk = 0;
    h->zero_off = 0;
    h->packed_total += 256;
    compute_f8ok(h);

    const int s_patch = h->add_spec("patch_embed.proj.weight", {F, 3, P, P});
    const int s_patch_b = h->add_spec("patch_embed.proj.bias", {F});
    w.patch = h->add_mat(s_patch, CLS_PATCH, MDPT_PACK_LINEAR, F, 3 * P * P, F, h->Kpatch, 0);
    w.patch_b = h->add_vec(s_patch_b, F, F);
    if (h->swin) {
        build_inventory_swin_encoder(h);
        build_inventory_decoder(h);
        return check_weight_refs(h);
    }

    const bool beit = is_beit(h);
    const int nlut = (2 * h->cfg.base_patch_grid_h - 1) * (2 * h->cfg.base_patch_grid_w - 1) + 3;
    w.cls_token = h->add_vec(h->add_spec("imgencoder.cls_token", {1, 1, F}), F, F);
    if (!beit) {
        const int s_cls = h->add_spec("imgencoder.posenc.cls_embedding", {1, 1, F});
        const int s_pos = h->add_spec("imgencoder.posenc.base_patch_embedding", {1, G, F});
        const int s_onw = h->add_spec("imgencoder.outnorm.weight", {F});
        const int s_onb = h->add_spec("imgencoder.outnorm.bias", {F});
        w.pos_cls = h->add_vec(s_cls, F, F);
        w.pos_patch = h->add_vec(s_pos, G * F, G * F);
        w.outnorm_w = h->add_vec(s_onw, F, F);
        w.outnorm_b = h->add_vec(s_onb, F, F);
    }

    // LayerScale (x + gamma * f(x), transformer_block.py:58,63) is folded into the producing Linear at pack time: rows of W and the
    // bias are multiplied by gamma, so the residual GEMMs compute out = (x + a W'^T) + b' with accumulators that START at x
    auto fold_layer_scale = [h](MatRef m, int s_gamma) {
        Mat& mm = h->mats[m.i];
        mm.row_scale = s_gamma;
#ifndef MDPT_NO_WSCALE  // (A/B builds)
        if (h->f16) {  // fp16 operands: a power-of-two factor keeps gamma * W (and its lo plane) in fp16's normal range (GemmParams::wscale)
            mm.off_scale = h->packed_total;
            h->packed_total += 256;
        }
#endif
    };
    // the MLP: Linear - GELU - Linear, or ViT-G's SwiGLU FFN (components/misc_helpers.py:162-168)
    const int sh = h->gh_hidden;
    const char* fc1_name = sh ? ".mlp.inner_linear_doubled" : ".mlp.layers.0";
    const char* fc2_name = sh ? ".mlp.outer_linear" : ".mlp.layers.2";
    const int fc1_n = sh ? 2 * sh : 4 * F, fc2_k = sh ? sh : 4 * F, fc2_kp = sh ? h->gh_hidden_p : 4 * F;
    for (int b = 0; b < h->nblocks; ++b) {
        const std::string p = blk_name(h, b);
        BlockRefs r;
        const int s_n1w = h->add_spec(p + ".norm1.weight", {F}), s_n1b = h->add_spec(p + ".norm1.bias", {F});
        r.ln1_w = h->add_vec(s_n1w, F, F);
        r.ln1_b = h->add_vec(s_n1b, F, F);
        const int s_n2w = h->add_spec(p + ".norm2.weight", {F}), s_n2b = h->add_spec(p + ".norm2.bias", {F});
        r.ln2_w = h->add_vec(s_n2w, F, F);
        r.ln2_b = h->add_vec(s_n2b, F, F);
        const int s_qkv = h->add_spec(p + ".attn.qkv.weight", {3 * F, F});
        int s_qkv_b = -1, s_q_b = -1, s_v_b = -1;
        if (beit) {  // qkv Linear has no bias; q and v get separate biases, k none (v31_beit/image_encoder_model.py:296-297,341-342)
            s_q_b = h->add_spec(p + ".attn.q_bias", {1, h->heads, 1, 64});
            s_v_b = h->add_spec(p + ".attn.v_bias", {1, h->heads, 1, 64});
            r.relpos_lut = h->add_vec(h->add_spec(p + ".attn.relpos_enc.ref_bias_lut", {nlut, h->heads}), nlut * h->heads, nlut * h->heads);
        } else {
            s_qkv_b = h->add_spec(p + ".attn.qkv.bias", {3 * F});
        }
        const int s_proj = h->add_spec(p + ".attn.proj.weight", {F, F});
        const int s_proj_b = h->add_spec(p + ".attn.proj.bias", {F});
        const int s_scale_attn = h->add_spec(p + ".scale_attn", {F});
        const int s_fc1 = h->add_spec(p + fc1_name + ".weight", {fc1_n, F});
        const int s_fc1_b = h->add_spec(p + fc1_name + ".bias", {fc1_n});
        const int s_fc2 = h->add_spec(p + fc2_name + ".weight", {F, fc2_k});
        const int s_fc2_b = h->add_spec(p + fc2_name + ".bias", {F});
        const int s_scale_mlp = h->add_spec(p + ".scale_mlp", {F});
        r.qkv = h->add_mat(s_qkv, CLS_QKV, MDPT_PACK_LINEAR, 3 * F, F, 3 * F, F, 0);
        r.proj = h->add_mat(s_proj, CLS_PROJ, MDPT_PACK_LINEAR, F, F, F, F, 0);
        r.fc1 = h->add_mat(s_fc1, CLS_FC1, MDPT_PACK_LINEAR, fc1_n, F, fc1_n, F, 0);
        r.fc2 = h->add_mat(s_fc2, CLS_FC2, MDPT_PACK_LINEAR, F, fc2_k, F, fc2_kp, 0);
        r.fc1_b = h->add_vec(s_fc1_b, fc1_n, fc1_n);
        fold_layer_scale(r.proj, s_scale_attn);
        fold_layer_scale(r.fc2, s_scale_mlp);
        r.proj_b = h->add_vec(s_proj_b, F, F, VEC_SCALED, s_scale_attn);
        r.fc2_b = h->add_vec(s_fc2_b, F, F, VEC_SCALED, s_scale_mlp);
        r.qkv_b = beit ? h->add_vec(s_q_b, 0, 3 * F, VEC_QV_BIAS, s_v_b) : h->add_vec(s_qkv_b, 3 * F, 3 * F);
        w.blocks.push_back(r);
    }

    for (int i = 0; i < 4; ++i) {
        const std::string p = std::string("reassemble.") + kStageNames[i];
        const int hd = h->hid[i], hp = h->hidp[i];
        auto& r = w.reasm[i];
        if (beit) {  // ReadoutProjectLayer: cat(token, cls) -> Linear(2F->F) -> GELU (components/readout_projection.py:42-46)
            const int s_ro = h->add_spec(p + ".readout_proj.1.weight", {F, 2 * F});
            const int s_ro_b = h->add_spec(p + ".readout_proj.1.bias", {F});
            r.readout_tok = h->add_mat(s_ro, CLS_REASM, MDPT_PACK_LINEAR, F, F, F, F, 0, 2 * F, 0);  // token half (columns 0..F)
            r.readout_cls = h->add_mat(s_ro, CLS_REASM, MDPT_PACK_LINEAR, F, F, F, F, 0, 2 * F, F);  // cls half (columns F..2F)
            r.readout_b = h->add_vec(s_ro_b, F, F);
        }
        const int s_r0 = h->add_spec(p + ".resample.0.weight", {hd, F, 1, 1});
        const int s_r0_b = h->add_spec(p + ".resample.0.bias", {hd});
        r.resample0 = h->add_mat(s_r0, CLS_REASM, MDPT_PACK_LINEAR, hd, F, hp, F, 0);
        r.resample0_b = h->add_vec(s_r0_b, hd, hp);
        if (i != 2) {  // ConvTranspose2d k == s (x4, x2) | 3x3 stride 2
            const int k = i == 0 ? 4 : (i == 1 ? 2 : 3);
            const int s_r1 = h->add_spec(p + ".resample.1.weight", {hd, hd, k, k});
            const int s_r1_b = h->add_spec(p + ".resample.1.bias", {hd});
            r.resample1 = i == 3 ? h->add_mat(s_r1, CLS_REASM, MDPT_PACK_CONV3, hd, hd, hp, 9 * hp, 3)
                                 : h->add_mat(s_r1, CLS_REASM, MDPT_PACK_CONVT, hd, hd, k * k * hp, hp, k);
            r.resample1_b = h->add_vec(s_r1_b, hd, hp);
        }
        r.fuse_proj = h->add_mat(h->add_spec(p + ".fuse_proj.weight", {h->C, hd, 3, 3}), CLS_REASM, MDPT_PACK_CONV3, h->C, hd, h->Cp, 9 * hp, 3);
    }
    build_inventory_decoder(h);
    return check_weight_refs(h);
}

// fusion + head parameters (same structure in every family; attribute names differ, see rcu_seq / proj_seq)
static void build_inventory_decoder(mdpt_handle* h) {
    const int C = h->C;
    for (int b = 0; b < 4; ++b) {
        char pb[64];
        snprintf(pb, sizeof(pb), "fusion.blocks.%d", b);
        const std::string unit[2] = {std::string(pb) + ".conv_reassembly", std::string(pb) + "." + proj_seq(h) + ".0"};
        for (int u = b < 3 ? 0 : 1; u < 2; ++u)  // the top-most block has no conv_reassembly unit
            for (int k = 0; k < 2; ++k) {
                const std::string n = unit[u] + "." + rcu_seq(h) + (k ? ".3" : ".1");
                const int s_w = h->add_spec(n + ".weight", {C, C, 3, 3});
                const int s_b = h->add_spec(n + ".bias", {C});
                h->w.fusion[b].rcu[u][k].w = h->add_mat(s_w, u ? CLS_FUSION : CLS_FUSION_IN, MDPT_PACK_CONV3, C, C, h->Cp, 9 * h->Cp, 3);
                h->w.fusion[b].rcu[u][k].b = h->add_vec(s_b, C, h->Cp);
            }
        const std::string o = std::string(pb) + "." + proj_seq(h) + ".2";
        const int s_w = h->add_spec(o + ".weight", {C, C, 1, 1});
        const int s_b = h->add_spec(o + ".bias", {C});
        h->w.fusion[b].proj = h->add_mat(s_w, CLS_FUSION_PROJ, MDPT_PACK_LINEAR, C, C, h->Cp, h->Cp, 0);
        h->w.fusion[b].proj_b = h->add_vec(s_b, C, h->Cp);
    }

    auto& hd = h->w.head;
    const int s_c1 = h->add_spec("head.spatial_upsampler.0.weight", {h->C2, C, 3, 3});
    const int s_c1_b = h->add_spec("head.spatial_upsampler.0.bias", {h->C2});
    const int s_p0 = h->add_spec("head.proj_1ch.0.weight", {32, h->C2, 3, 3});
    const int s_p0_b = h->add_spec("head.proj_1ch.0.bias", {32});
    const int s_p2 = h->add_spec("head.proj_1ch.2.weight", {1, 32, 1, 1});
    const int s_p2_b = h->add_spec("head.proj_1ch.2.bias", {1});
    hd.conv1 = h->add_mat(s_c1, CLS_HEAD, MDPT_PACK_CONV3, h->C2, C, h->C2p, 9 * h->Cp, 3);
    hd.conv1_b = h->add_vec(s_c1_b, h->C2, h->C2p);
    hd.proj0 = h->add_mat(s_p0, CLS_HEAD_TAIL, MDPT_PACK_CONV3, 32, h->C2, 32, 9 * h->C2p, 3);
    if (head_tail_fused(h))  // LDS image of the same weights for the fused head tail (head.hip)
        hd.proj0_kc32 = h->add_mat(s_p0, CLS_HEAD_TAIL, MDPT_PACK_CONV3_KC32, 32, h->C2, 32, 9 * h->C2p, 3);
    hd.proj0_b = h->add_vec(s_p0_b, 32, 32);
    hd.proj2_w = h->add_vec(s_p2, 32, 32);
    hd.proj2_b = h->add_vec(s_p2_b, 1, 4);
}

// Every reference the stage drivers of this configuration dereference exists: the drivers' family / ViT-G / fused-tail branches, restated once. A
// branch that differs between the inventory and a driver is an error of mdpt_create / mdpt_set_class_passes here, not a wild index in a forward.
static int check_weight_refs(const mdpt_handle* h) {
    const WeightRefs& w = h->w;
    const char* missing = nullptr;
    auto mat = [&](MatRef r, const char* what) { if (!missing && (r.i < 0 || r.i >= (int)h->mats.size())) missing = what; };
    auto vec = [&](VecRef r, const char* what) { if (!missing && (r.i < 0 || r.i >= (int)h->vecs.size())) missing = what; };
    const bool beit = is_beit(h), vit = !h->swin;
    mat(w.patch, "patch embedding"); vec(w.patch_b, "patch embedding bias");
    if (h->swin) { vec(w.patch_ln_w, "patch embedding norm"); vec(w.patch_ln_b, "patch embedding norm"); }
    if (vit) vec(w.cls_token, "cls token");
    if (vit && !beit) { vec(w.pos_cls, "position embedding"); vec(w.pos_patch, "position embedding"); vec(w.outnorm_w, "out norm"); vec(w.outnorm_b, "out norm"); }
    if ((int)w.blocks.size() != h->nblocks) return fail(MDPT_E_INVALID, "internal: the inventory holds %zu encoder blocks, the configuration %d", w.blocks.size(), h->nblocks);
    for (const BlockRefs& r : w.blocks) {
        mat(r.qkv, "block qkv"); mat(r.proj, "block proj"); mat(r.fc1, "block fc1"); mat(r.fc2, "block fc2");
        for (VecRef v : {r.ln1_w, r.ln1_b, r.ln2_w, r.ln2_b, r.qkv_b, r.proj_b, r.fc1_b, r.fc2_b}) vec(v, "block norm / bias");
        if (beit) vec(r.relpos_lut, "block relative-position table");
        if (h->swin) for (VecRef v : {r.logit_scale, r.cpb_w1, r.cpb_b1, r.cpb_w2}) vec(v, "block logit scale / position-bias MLP");
    }
    for (int s = 0; s < 3 && h->swin; ++s) { mat(w.merge[s].reduction, "patch merge"); vec(w.merge[s].norm_w, "patch merge norm"); vec(w.merge[s].norm_b, "patch merge norm"); }
    for (int i = 0; i < 4; ++i) {
        const auto& r = w.reasm[i];
        mat(r.fuse_proj, "reassembly fuse_proj");
        if (beit) { mat(r.readout_tok, "readout projection"); mat(r.readout_cls, "readout projection"); vec(r.readout_b, "readout projection bias"); }
        if (vit) { mat(r.resample0, "reassembly resample 0"); vec(r.resample0_b, "reassembly resample 0 bias"); }
        if (vit && i != 2) { mat(r.resample1, "reassembly resample 1"); vec(r.resample1_b, "reassembly resample 1 bias"); }
        for (int u = i < 3 ? 0 : 1; u < 2; ++u)
            for (int k = 0; k < 2; ++k) { mat(w.fusion[i].rcu[u][k].w, "fusion conv"); vec(w.fusion[i].rcu[u][k].b, "fusion conv bias"); }
        mat(w.fusion[i].proj, "fusion projection"); vec(w.fusion[i].proj_b, "fusion projection bias");
    }
    mat(w.head.conv1, "head conv 1"); vec(w.head.conv1_b, "head conv 1 bias"); mat(w.head.proj0, "head proj 0");
    if (head_tail_fused(h)) mat(w.head.proj0_kc32, "head proj 0 (fused tail image)");
    vec(w.head.proj0_b, "head proj 0 bias"); vec(w.head.proj2_w, "head proj 2"); vec(w.head.proj2_b, "head proj 2 bias");
    if (missing) return fail(MDPT_E_INVALID, "internal: the parameter inventory of this configuration has no %s", missing);
    return 0;
}

// ------------------------------------------------------------------------------------------------------------
// workspace planning
// ------------------------------------------------------------------------------------------------------------
// f8mode (fm() of the CONSUMING class): 0 = 16-bit residue plane, 1 = e5m2 residue bytes, 2 = + the e5m2 plane of the values (three terms);
// the buffer is the same 2 bytes per element either way (Planes, f8_cross.h)
void take_planes(Bump& bump, bool x3, size_t elems, size_t out[3], int f8mode = 0) {
    out[0] = bump.take(elems * 2);
    out[1] = x3 ? bump.take(elems * 2) : SIZE_MAX;
    out[2] = x3 && f8mode ? (elems | (f8mode == 2 ? (size_t)1 << 63 : 0)) : 0;
}
static int fm(const mdpt_handle* h, int cls) { return h->f8(cls) ? (h->terms(cls) == 3 ? 2 : 1) : 0; }

// reassembly outputs, fusion and head buffers; p.Np / p.gh / p.gw = the "noscale" level (1/Pv of the image)
void plan_decoder(Bump& bump, const mdpt_handle* h, Plan& p, size_t min_scratch_floats) {
    // lo planes exist where the CONSUMING class reads one (2 or 3 passes): the reassembly maps of levels 0..2 and a1 feed the conv_reassembly
    // units (CLS_FUSION_IN), level 3's map, x and b1 the projection path's 3x3 convs (CLS_FUSION), b2 the 1x1 projection (CLS_FUSION_PROJ)
    const bool x3 = h->alo(CLS_FUSION), x3i = h->alo(CLS_FUSION_IN), x3p = h->alo(CLS_FUSION_PROJ), x3h = h->alo(CLS_HEAD);
    const int B = p.B;
    const size_t px[4] = {(size_t)16 * p.Np, (size_t)4 * p.Np, (size_t)p.Np, (size_t)p.Np / 4};
    for (int i = 0; i < 4; ++i) {
        const size_t e = (size_t)B * px[i] * h->Cp;
        p.r_f32[i] = bump.take(e * 4);
        take_planes(bump, i == 3 ? x3 : x3i, e, p.r_bf[i], fm(h, i == 3 ? CLS_FUSION : CLS_FUSION_IN));
        take_planes(bump, x3i, e, p.a1[i], fm(h, CLS_FUSION_IN));
        p.x_f32[i] = bump.take(e * 4);
        take_planes(bump, x3, e, p.x_bf[i], fm(h, CLS_FUSION));
        take_planes(bump, x3, e, p.b1[i], fm(h, CLS_FUSION));
        take_planes(bump, x3p, e, p.b2[i], fm(h, CLS_FUSION_PROJ));
        p.flo[i] = bump.take(e * 4);
    }
    const size_t fpx = (size_t)64 * p.Np;  // (8gh)*(8gw)
    take_planes(bump, x3h, (size_t)B * fpx * h->Cp, p.fused, fm(h, CLS_HEAD));
    // bf16 mode with the fused head tail (run_head): conv 1 writes a bf16 map and the full-resolution upsampled map never exists (ViT-L,
    // 504x504, batch 32: 2.1 GB + 0.7 GB of workspace that used to be reserved and never touched)
    const bool bf16_head = head_tail_fused(h) && mdpt_head_tail_scale_ok(8 * p.gh, 8 * p.gw, p.H, p.W);
    p.h1 = bump.take((size_t)B * fpx * h->C2p * (bf16_head && h->terms(CLS_HEAD_TAIL) == 1 ? 2 : 4));  // one 16-bit plane | hi + lo planes | fp32 map
    if (bf16_head) p.h1u[0] = p.h1u[1] = SIZE_MAX;
    else take_planes(bump, h->alo(CLS_HEAD_TAIL), (size_t)B * p.H * p.W * h->C2p, p.h1u);
    p.scratch_floats = (size_t)B * fpx * h->Cp;
    if (min_scratch_floats > p.scratch_floats) p.scratch_floats = min_scratch_floats;
    p.scratch = bump.take(p.scratch_floats * 4);
    p.probe = bump.take(256);  // the side-stream probe's two flag words: nothing else ever lives here (mdpt_api.cpp ensure_side_stream)
    p.poison = bump.take((size_t)p.B * 4);  // per-image non-finite flags (patchify_kernel sets, poison_depth_kernel reads: mdpt_api.cpp forward_one)
}

int make_plan_swin(const mdpt_handle* h, int B, int H, int W, Plan* pl);

int make_plan(const mdpt_handle* h, int B, int H, int W, Plan* pl) {
    if (B <= 0 || H <= 0 || W <= 0) return fail(MDPT_E_INVALID, "bad batch/size B=%d H=%d W=%d", B, H, W);
    if (h->swin) return make_plan_swin(h, B, H, W, pl);
    if (H % h->P || W % h->P)
        return fail(MDPT_E_INVALID, "image size %dx%d must be divisible by the patch size %d (reference patch_embed.py:159-163)", H, W, h->P);
    const int gh = H / h->P, gw = W / h->P;
    if ((gh & 1) || (gw & 1))
        return fail(MDPT_E_GRID, "patch grid %dx%d must be even in both dimensions (the reference fails in fusion_model.py:151)", gh, gw);
    const int F = h->F;
    Plan& p = *pl;
    p.B = B; p.H = H; p.W = W; p.gh = gh; p.gw = gw;
    p.Np = gh * gw; p.N = p.Np + 1; p.npad = rup(p.N, 8); p.npadv = rup(p.N, 64);
    Bump bump;
    const size_t rows = (size_t)B * p.npad;
    take_planes(bump, h->alo(CLS_PATCH), (size_t)B * p.Np * h->Kpatch, p.im2col);
    p.pos = bump.take((size_t)p.Np * F * 4);
    p.resid = bump.take(rows * F * 4);
    take_planes(bump, h->alo(CLS_QKV) || h->alo(CLS_FC1), rows * F, p.xn);
    take_planes(bump, h->x3c(CLS_ATTN), (size_t)B * h->heads * p.npad * 64, p.q);
    take_planes(bump, h->x3c(CLS_ATTN), (size_t)B * h->heads * p.npad * 64, p.k);
    take_planes(bump, h->x3c(CLS_ATTN), (size_t)B * h->heads * 64 * p.npadv, p.vt);
    take_planes(bump, h->alo(CLS_PROJ) || h->x3c(CLS_ATTN), rows * F, p.att);  // the 3-pass attention kernel always writes its lo plane
    take_planes(bump, h->alo(CLS_FC2), rows * 4 * F, p.hbuf);
    p.swi = h->gh_hidden ? bump.take(rows * 2 * h->gh_hidden * 4) : SIZE_MAX;
    p.kspart = fc2_ksplit_fits((int)rows, F) ? bump.take(rows * F * 4 * 3) : SIZE_MAX;  // three partial-sum planes (a split in four); reserved whatever the latency switch says: it may flip later
    p.wrc_mean = h->wrc_maxk ? bump.take((size_t)B * h->wrc_maxk * 2) : SIZE_MAX;
    p.wrc_tab = h->wrc_maxn ? bump.take((size_t)B * h->wrc_maxn * 4) : SIZE_MAX;
    const bool x3 = h->alo(CLS_REASM);
    const int fr = fm(h, CLS_REASM);
    for (int i = 0; i < 4; ++i) take_planes(bump, x3, rows * F, p.tap[i], fr);
    p.tapf32 = bump.take(rows * F * 4);
    const size_t px[4] = {(size_t)16 * p.Np, (size_t)4 * p.Np, (size_t)p.Np, (size_t)p.Np / 4};
    for (int i = 0; i < 4; ++i) take_planes(bump, x3, (size_t)B * p.Np * h->hidp[i], p.t[i], fr);
    take_planes(bump, x3, (size_t)B * px[0] * h->hidp[0], p.u0, fr);
    take_planes(bump, x3, (size_t)B * px[1] * h->hidp[1], p.u1, fr);
    take_planes(bump, x3, (size_t)B * px[3] * h->hidp[3], p.d3, fr);
    plan_decoder(bump, h, p, rows * F);
    p.tokr[0] = p.tokr[1] = p.cbuf = p.relpos_lut = p.relpos_tq = p.relpos_tk = SIZE_MAX;
    if (is_beit(h)) {
        take_planes(bump, x3, (size_t)B * p.Np * F, p.tokr, fr);
        p.cbuf = bump.take((size_t)B * F * 4);
        p.relpos_lut = bump.take((size_t)h->heads * mdpt_beit_relpos_elen(gh, gw) * 4 * (h->nblocks <= 32 ? h->nblocks : 1));  // one table per block
        p.relpos_tq = bump.take((size_t)p.npadv * 4);
        p.relpos_tk = bump.take((size_t)p.npadv * 4);
    }
    p.total = bump.off;
    return 0;
}

#include "mdpt_swin_plan.inc"

int check_ws(const mdpt_handle* h, const Plan& p, const void* ws, size_t bytes) {
    if (!h->finalized) return fail(MDPT_E_STATE, "mdpt_finalize() has not been called");
    if (!ws || bytes < p.total) return fail(MDPT_E_WORKSPACE, "workspace too small: need %zu bytes, got %zu", p.total, bytes);
    if (((uintptr_t)ws) & 255) return fail(MDPT_E_WORKSPACE, "workspace must be 256-byte aligned");
    return 0;
}

int make_ctx(mdpt_handle* h, int B, int H, int W, void* ws, size_t ws_bytes, void* stream, Ctx* c) {
    Plan p;
    CHK(make_plan(h, B, H, W, &p));
    CHK(check_ws(h, p, ws, ws_bytes));
    c->h = h; c->p = p; c->ws = (char*)ws; c->s = (hipStream_t)stream;
    h->cache_clear();  // whoever builds a context may write the constant regions for another grid (stage-level calls): mdpt_forward re-validates its own
    return 0;
}

}  // namespace mdpt
