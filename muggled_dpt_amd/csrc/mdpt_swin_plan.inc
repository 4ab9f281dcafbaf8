// SwinV2 (MiDaS v3.1) encoder: stage geometry, parameter inventory and workspace plan; included by mdpt_inventory.cpp inside namespace mdpt
// (the stage drivers are in mdpt_swin_stages.inc).
//
// Reference: muggled_dpt/v31_swinv2/image_encoder_model.py:77-98 (4 stages + 3 patch merges), :213-225 (post-norm block),
// components/windowed_attention.py:65-123 (window cosine attention), :345-388 (window / shift sizes per grid),
// components/patch_merge.py:49-103, patch_embed.py:76-94 (conv k4 s4 + LayerNorm), reassembly_model.py:113-122.
//
// Layout: stage s keeps its tokens as a dense fp32 residual stream [B, gh_s*gw_s, F_s] (no cls token, no row padding), which
// is also NHWC [B, gh_s, gw_s, F_s] - the reassembly 3x3 conv reads the bf16 copy of it directly. Window partition, the
// cyclic shift and their inverses are never materialised on the token stream: swin_qkv_prep gathers through the window map
// and the attention kernel scatters its output rows back through the same map.

// adjust_window_and_shift_sizes (windowed_attention.py:345-388)
int swin_window_for(int patch, int target, int* win, int* shift) {
    int w = target < patch ? target : patch;
    if (patch % w) {
        int best = -1;
        for (int div = w / 2; div < 2 * w; ++div) {
            if (div <= 0 || patch % div) continue;
            if (best < 0 || abs(patch - div) < abs(patch - best)) best = div;
        }
        if (best < 0) return fail(MDPT_E_INVALID, "no window size in [%d, %d) tiles a patch grid side of %d (the reference raises ValueError)", w / 2, 2 * w, patch);
        w = best;
    }
    *win = w;
    *shift = patch <= w ? 0 : w / 2;
    return 0;
}

int swin_geom(const mdpt_handle* h, int g0h, int g0w, int s, SwinStageGeom* g) {
    g->gh = g0h >> s; g->gw = g0w >> s;
    g->N = g->gh * g->gw;
    g->F = h->hid[s]; g->heads = h->sH[s];
    CHK(swin_window_for(g->gh, h->swh, &g->wh, &g->sh));
    CHK(swin_window_for(g->gw, h->sww, &g->ww, &g->sw));
    g->nw = (g->gh / g->wh) * (g->gw / g->ww);
    g->wa = g->wh * g->ww;
    g->npad = rup(g->wa, 8);
    g->npadv = rup(g->wa, 64);
    return 0;
}

static void build_inventory_swin_encoder(mdpt_handle* h) {
    WeightRefs& w = h->w;
    const int s_ln_w = h->add_spec("patch_embed.norm.weight", {h->F});
    const int s_ln_b = h->add_spec("patch_embed.norm.bias", {h->F});
    w.patch_ln_w = h->add_vec(s_ln_w, h->F, h->F);
    w.patch_ln_b = h->add_vec(s_ln_b, h->F, h->F);
    for (int s = 0; s < 4; ++s) {
        const int F = h->hid[s], H = h->sH[s];
        for (int l = 0; l < h->sL[s]; ++l) {
            char buf[96];
            snprintf(buf, sizeof(buf), "imgencoder.stages.%d.blocks.%d", s, l);
            const std::string p = buf;
            BlockRefs r;
            const int s_q_b = h->add_spec(p + ".attn.q_bias", {1, H, 1, 32});
            const int s_v_b = h->add_spec(p + ".attn.v_bias", {1, H, 1, 32});
            const int s_qkv = h->add_spec(p + ".attn.qkv.weight", {3 * F, F});
            const int s_ls = h->add_spec(p + ".attn.logit_scale", {H, 1, 1});
            const int s_cpb_w1 = h->add_spec(p + ".attn.relpos_enc.bias_mlp.0.weight", {kCpbHidden, 2});
            const int s_cpb_b1 = h->add_spec(p + ".attn.relpos_enc.bias_mlp.0.bias", {kCpbHidden});
            const int s_cpb_w2 = h->add_spec(p + ".attn.relpos_enc.bias_mlp.2.weight", {H, kCpbHidden});
            const int s_proj = h->add_spec(p + ".attn.proj.weight", {F, F});
            const int s_proj_b = h->add_spec(p + ".attn.proj.bias", {F});
            const int s_n1w = h->add_spec(p + ".norm1.weight", {F});
            const int s_n1b = h->add_spec(p + ".norm1.bias", {F});
            const int s_fc1 = h->add_spec(p + ".mlp.layers.0.weight", {4 * F, F});
            const int s_fc1_b = h->add_spec(p + ".mlp.layers.0.bias", {4 * F});
            const int s_fc2 = h->add_spec(p + ".mlp.layers.2.weight", {F, 4 * F});
            const int s_fc2_b = h->add_spec(p + ".mlp.layers.2.bias", {F});
            const int s_n2w = h->add_spec(p + ".norm2.weight", {F});
            const int s_n2b = h->add_spec(p + ".norm2.bias", {F});
            r.qkv = h->add_mat(s_qkv, CLS_QKV, MDPT_PACK_LINEAR, 3 * F, F, 3 * F, rup(F, 64), 0);
            r.proj = h->add_mat(s_proj, CLS_PROJ, MDPT_PACK_LINEAR, F, F, F, rup(F, 64), 0);
            r.fc1 = h->add_mat(s_fc1, CLS_FC1, MDPT_PACK_LINEAR, 4 * F, F, 4 * F, rup(F, 64), 0);
            r.fc2 = h->add_mat(s_fc2, CLS_FC2, MDPT_PACK_LINEAR, F, 4 * F, F, 4 * F, 0);
            r.qkv_b = h->add_vec(s_q_b, 0, 3 * F, VEC_QV_BIAS, s_v_b);
            r.logit_scale = h->add_vec(s_ls, H, H, VEC_LOG2E);
            r.cpb_w1 = h->add_vec(s_cpb_w1, 2 * kCpbHidden, 2 * kCpbHidden);
            r.cpb_b1 = h->add_vec(s_cpb_b1, kCpbHidden, kCpbHidden);
            r.cpb_w2 = h->add_vec(s_cpb_w2, H * kCpbHidden, H * kCpbHidden);
            r.proj_b = h->add_vec(s_proj_b, F, F);
            r.ln1_w = h->add_vec(s_n1w, F, F);
            r.ln1_b = h->add_vec(s_n1b, F, F);
            r.fc1_b = h->add_vec(s_fc1_b, 4 * F, 4 * F);
            r.fc2_b = h->add_vec(s_fc2_b, F, F);
            r.ln2_w = h->add_vec(s_n2w, F, F);
            r.ln2_b = h->add_vec(s_n2b, F, F);
            w.blocks.push_back(r);
        }
        if (s < 3) {
            char pm[96];
            snprintf(pm, sizeof(pm), "imgencoder.patch_merge_layers.%d", s);
            const int Fo = h->hid[s + 1];
            const int s_red = h->add_spec(std::string(pm) + ".reduction.weight", {Fo, 4 * F});
            const int s_nw = h->add_spec(std::string(pm) + ".norm.weight", {Fo});
            const int s_nb = h->add_spec(std::string(pm) + ".norm.bias", {Fo});
            w.merge[s].reduction = h->add_mat(s_red, CLS_PROJ, MDPT_PACK_LINEAR, Fo, 4 * F, Fo, 4 * F, 0);  // a token-mixing projection
            w.merge[s].norm_w = h->add_vec(s_nw, Fo, Fo);
            w.merge[s].norm_b = h->add_vec(s_nb, Fo, Fo);
        }
    }
    for (int s = 0; s < 4; ++s) {
        const std::string p = std::string("reassemble.") + kSwinStageNames[s];
        w.reasm[s].fuse_proj = h->add_mat(h->add_spec(p + ".fuse_proj.weight", {h->C, h->hid[s], 3, 3}), CLS_REASM, MDPT_PACK_CONV3, h->C, h->hid[s], h->Cp,
                                          9 * h->hidp[s], 3);
    }
}

int make_plan_swin(const mdpt_handle* h, int B, int H, int W, Plan* pl) {
    if (H % h->P || W % h->P)
        return fail(MDPT_E_INVALID, "image size %dx%d must be divisible by the patch size %d (reference patch_embed.py:156-160)", H, W, h->P);
    const int g0h = H / h->P, g0w = W / h->P;
    if ((g0h & 7) || (g0w & 7))
        return fail(MDPT_E_GRID, "patch grid %dx%d must be divisible by 8 (three 2x2 patch merges; the reference fails in "
                                 "patch_merge.py:91 / fusion_model.py otherwise)", g0h, g0w);
    Plan& p = *pl;
    memset(&p, 0xff, sizeof(p));  // every offset SIZE_MAX (= absent) unless taken below
    p.B = B; p.H = H; p.W = W;
    p.gh = g0h / 4; p.gw = g0w / 4;  // the "noscale" level of the decoder pyramid
    p.Np = p.gh * p.gw; p.N = p.Np; p.npad = p.Np; p.npadv = rup(p.Np, 64);
    p.sw.g0h = g0h; p.sw.g0w = g0w;
    Bump bump;
    size_t max_x = 0, max_tok = 0, max_qk = 0, max_vt = 0, max_lut = 0, max_n = 0, max_tk = 0;
    for (int s = 0; s < 4; ++s) {
        SwinStageGeom g;
        CHK(swin_geom(h, g0h, g0w, s, &g));
        if (g.heads * 32 != g.F) return fail(MDPT_E_UNSUPPORTED, "SwinV2 stage %d: head dim must be 32 (features %d, heads %d)", s, g.F, g.heads);
        const size_t rows = (size_t)B * g.N;
        p.sw.resid[s] = bump.take(rows * g.F * 4);
        take_planes(bump, h->alo(CLS_REASM), rows * (size_t)rup(g.F, 64), p.tap[s]);  // operand planes: rows padded to a multiple of 64 columns
        if (rows * 3 * g.F > max_x) max_x = rows * 3 * g.F;
        if (rows * (size_t)rup(g.F, 64) > max_tok) max_tok = rows * (size_t)rup(g.F, 64);
        const size_t qk = (size_t)B * g.nw * g.heads * g.npad * 32, vt = (size_t)B * g.nw * g.heads * 32 * g.npadv;
        if (qk > max_qk) max_qk = qk;
        if (vt > max_vt) max_vt = vt;
        const size_t lut = (size_t)g.heads * (2 * g.wh - 1) * (2 * g.ww - 1);
        if (lut > max_lut) max_lut = lut;
        if ((size_t)g.N > max_n) max_n = g.N;
        if ((size_t)g.npadv > max_tk) max_tk = g.npadv;
    }
    take_planes(bump, h->alo(CLS_PATCH), (size_t)B * g0h * g0w * h->Kpatch, p.im2col);
    p.sw.x = bump.take(max_x * 4);
    take_planes(bump, h->alo(CLS_QKV) || h->alo(CLS_FC1) || h->alo(CLS_PROJ), max_tok, p.sw.xn);  // QKV / fc1 / patch-merge operand
    take_planes(bump, h->x3c(CLS_ATTN), max_qk, p.sw.q);
    take_planes(bump, h->x3c(CLS_ATTN), max_qk, p.sw.k);
    take_planes(bump, h->x3c(CLS_ATTN), max_vt, p.sw.vt);
    take_planes(bump, h->alo(CLS_PROJ) || h->x3c(CLS_ATTN), max_tok, p.sw.att);
    take_planes(bump, h->alo(CLS_FC2), max_tok * 4, p.sw.hb);
    int nblocks = 0;
    for (int s = 0; s < 4; ++s) nblocks += h->sL[s];
    p.sw.lut_stride = max_lut * 4;
    p.sw.lut = bump.take(p.sw.lut_stride * (size_t)nblocks);  // one LUT per block, all filled by one launch per forward
    p.sw.tq = bump.take(max_tk * 4);
    p.sw.tk = bump.take(max_tk * 4);
    for (int v = 0; v < 2; ++v) {
        p.sw.rowmap[v] = bump.take(max_n * 4);
        p.sw.region[v] = bump.take(max_n * 4);
        p.sw.tokmap[v] = bump.take(max_n * 4);
        p.sw.vtokmap[v] = bump.take(max_n * 4);
    }
    p.wrc_mean = h->wrc_maxk ? bump.take((size_t)B * h->wrc_maxk * 2) : SIZE_MAX;
    p.wrc_tab = h->wrc_maxn ? bump.take((size_t)B * h->wrc_maxn * 4) : SIZE_MAX;
    p.kspart = SIZE_MAX;
    plan_decoder(bump, h, p, 0);
    p.total = bump.off;
    return 0;
}

