// SwinV2 (MiDaS v3.1) encoder stage drivers; included by mdpt_stages.cpp inside namespace mdpt (geometry / inventory / plan: mdpt_swin_plan.inc).

// A first stage that is not a multiple of 64 wide (swin2_tiny_256: 96) keeps its bf16 operand planes (LN output, attention output,
// stage tap) at a row stride of roundup(F, 64); the pad columns meet zero weight columns in the GEMMs and must be zero themselves:
// cleared here once per forward, the producers only ever write the F real columns. Later stages double the width (multiples of 64).
int swin_zero_pad_planes(const Ctx& c, int rows0) {
    const mdpt_handle* h = c.h;
    const int F = h->hid[0], Fp = rup(F, 64);
    if (Fp == F) return 0;
    const size_t bytes = (size_t)rows0 * Fp * 2;
    for (size_t off : {c.p.sw.xn[0], c.p.sw.xn[1], c.p.sw.att[0], c.p.sw.att[1], c.p.tap[0][0], c.p.tap[0][1]})
        if (off != SIZE_MAX) CHK(hipMemsetAsync(c.ws + off, 0, bytes, c.s));
    return 0;
}

// conv k4 s4 + LayerNorm(eps 1e-5) -> stage-0 residual stream (+ bf16 token planes in sw.xn)
int run_patch_embed_swin(const Ctx& c, const void* image, int image_dtype, float* tokens_out) {
    const mdpt_handle* h = c.h;
    const Plan& p = c.p;
    const int rows = p.B * p.sw.g0h * p.sw.g0w;
    Planes im = c.pl(p.im2col);
    CHK(run_patchify(c, image, image_dtype, im, p.sw.g0h * h->P, p.sw.g0w * h->P));
    GemmParams g = base_params(c, h->M(h->w.patch), im, rows, h->Kpatch);
    g.bias = h->V(h->w.patch_b);
    g.out_f32 = c.at<float>(p.sw.x); g.ldc = h->F;
    CHK(OPLC(mdpt_launch_gemm, g, c.s));
    Planes xn = c.pl(p.sw.xn);
    float* out = tokens_out ? tokens_out : c.at<float>(p.sw.resid[0]);
    if (!tokens_out) CHK(swin_zero_pad_planes(c, rows));
    CHK(OPLC(mdpt_launch_ln_res, c.at<float>(p.sw.x), nullptr, h->V(h->w.patch_ln_w), h->V(h->w.patch_ln_b), 1e-5f, out,
                           tokens_out ? nullptr : xn.hi, tokens_out ? nullptr : xn.lo, rows, h->F, c.s, rup(h->F, 64)));
    return 0;
}

// the four stages; expects resid[0] (fp32) and sw.xn (its bf16 planes) filled. taps_f32 != null: copy the stage outputs out.
// K split of fc2 where K is long (>= 3072: the late stages, few tiles per launch): two ranges of an even number of K tiles. (The attention projection
// of the same stages, K = F = 768 -> 6 + 6 K tiles, measured: no gain - SwinV2-L 2.004 x the ViT-L rate of the box against 2.016 without.)
static inline bool swin_ksplit(int F, int K) { (void)F; return K >= 3072 && (K / 64) % 4 == 0; }

int run_encoder_swin(const Ctx& c, void* const taps_f32[4]) {
    const mdpt_handle* h = c.h;
    const Plan& p = c.p;
    Planes xn = c.pl(p.sw.xn), q = c.pl(p.sw.q), k = c.pl(p.sw.k), vt = c.pl(p.sw.vt), att = c.pl(p.sw.att), hb = c.pl(p.sw.hb);
    float* x = c.at<float>(p.sw.x);
    if (!c.consts_cached) {   // continuous-position-bias tables of every block: weights and window geometry only -> one batched launch up front (once per grid with the cache)
        SwinCpbBatch cb;
        memset(&cb, 0, sizeof(cb));
        cb.hidden = kCpbHidden;
        for (int s = 0; s < 4; ++s) {
            SwinStageGeom g;
            CHK(swin_geom(h, p.sw.g0h, p.sw.g0w, s, &g));
            for (int l = 0; l < h->sL[s]; ++l) {
                if (cb.n >= 32) return fail(MDPT_E_UNSUPPORTED, "more than 32 SwinV2 blocks");
                const BlockRefs& w = h->w.blocks[cb.n];
                cb.w1[cb.n] = h->V(w.cpb_w1);
                cb.b1[cb.n] = h->V(w.cpb_b1);
                cb.w2[cb.n] = h->V(w.cpb_w2);
                cb.lut[cb.n] = (float*)(c.ws + p.sw.lut + (size_t)cb.n * p.sw.lut_stride);
                cb.heads[cb.n] = g.heads; cb.wh[cb.n] = g.wh; cb.ww[cb.n] = g.ww; cb.pre[cb.n] = h->spre[s];
                ++cb.n;
            }
        }
        CHK(OPLC(mdpt_launch_swin_cpb_batch, cb, c.s));
    }
    int blk_index = 0;
    for (int s = 0; s < 4; ++s) {
        SwinStageGeom g;
        CHK(swin_geom(h, p.sw.g0h, p.sw.g0w, s, &g));
        const int F = g.F, Fp = rup(g.F, 64), rows = p.B * g.N;
        float* resid = c.at<float>(p.sw.resid[s]);
        // 3-pass projection behind the 1-pass attention kernel (no lo plane written): zero plane, see run_encoder
        if (att.lo && !h->x3c(CLS_ATTN)) CHK(hipMemsetAsync(att.lo, 0, (size_t)rows * Fp * 2, c.s));
        const bool shifting = g.sh > 0 || g.sw > 0;
        int* rowmap[2] = {c.at<int>(p.sw.rowmap[0]), c.at<int>(p.sw.rowmap[1])};
        int* region[2] = {c.at<int>(p.sw.region[0]), c.at<int>(p.sw.region[1])};
        int* tokmap[2] = {c.at<int>(p.sw.tokmap[0]), c.at<int>(p.sw.tokmap[1])};
        int* vtokmap[2] = {c.at<int>(p.sw.vtokmap[0]), c.at<int>(p.sw.vtokmap[1])};
        CHK(OPLC(mdpt_launch_swin_window_map, rowmap[0], region[0], c.at<int>(p.sw.tq), c.at<int>(p.sw.tk), g.gh, g.gw, g.wh, g.ww, 0, 0, g.wa,
                                        g.npadv, c.s, tokmap[0], g.heads * g.npad, vtokmap[0], g.heads * 32 * g.npadv));
        if (shifting)
            CHK(OPLC(mdpt_launch_swin_window_map, rowmap[1], region[1], c.at<int>(p.sw.tq), c.at<int>(p.sw.tk), g.gh, g.gw, g.wh, g.ww, g.sh, g.sw,
                                            g.wa, g.npadv, c.s, tokmap[1], g.heads * g.npad, vtokmap[1], g.heads * 32 * g.npadv));
        // Q / K straight out of the QKV GEMM's accumulators (gemm.hip epilogue_swin_qk) when its 256-column tiles do not straddle the
        // K | V boundary, the planes fit 32-bit offsets and the tile rule picks the 8-phase kernel; otherwise fp32 QKV rows + swin_qk_prep.
        // Both forms give the same bits (same arithmetic in the same order), so the choice may depend on the batch size.
        const size_t img_rows = (size_t)g.nw * g.heads * g.npad;
        // V likewise (epilogue_swin_vt) when runs of 4 tokens stay together; the pad positions [wa, npadv) of Vt, which swin_v_prep writes
        // as zeros on every call, are zeroed once per stage then
        const size_t img_velems = (size_t)g.nw * g.heads * 32 * g.npadv;
        const bool v_direct_ok = g.gw % 4 == 0 && g.ww % 4 == 0 && g.sw % 4 == 0 && (size_t)p.B * img_velems * 2 < 0xFFFFFFF0ull;
        bool vt_zeroed = false;
        const bool qk_planes_ok = (2 * F) % 256 == 0 && (size_t)p.B * img_rows * 64 < 0xFFFFFFF0ull && (size_t)p.B * img_rows < 0x7FFFFFFFull;
        for (int l = 0; l < h->sL[s]; ++l) {
            const BlockRefs& w = h->w.blocks[blk_index];
            const int v = (l & 1) && shifting ? 1 : 0;  // odd blocks of a pair are the shifted ones (image_encoder_model.py:155-161)
            bool qk_fused = false, v_fused = false;
            {
                GemmParams gm = base_params(c, h->M(w.qkv), xn, rows, Fp);
                gm.bias = h->V(w.qkv_b);
                gm.out_f32 = x; gm.ldc = 3 * F;
#ifdef MDPT_DEBUG_SWITCHES  // A/B builds only (tests force the unfused forms through mdpt_set_gemm_tile)
                static const bool no_fusion = getenv("MDPT_SWIN_NO_QK_FUSION") != nullptr;
                static const bool no_fusion_v = getenv("MDPT_SWIN_NO_V_FUSION") != nullptr;
#else
                constexpr bool no_fusion = false, no_fusion_v = false;
#endif
                // token-mean compensation of the weight rounding (fp16 modes): per-image bias table; the fused Q / K / V epilogues take it for
                // stages of >= 256 tokens per image (two images per tile at most), smaller stages keep the fp32 rows + prep kernels
                CHK(wrc_bias(c, gm, h->M(w.qkv), gm.bias, g.N, g.N));
                qk_fused = !no_fusion && qk_planes_ok && Fp == F && (!gm.bias_img_stride || g.N >= 256) && OPLC(mdpt_gemm_resolves_to_pp256, gm);
                if (qk_fused) {
                    gm.ekind = MDPT_E_SWQKV;
                    gm.F = F; gm.heads = g.heads; gm.npad = g.npad; gm.npadv = g.npadv;
                    gm.q_hi = q.hi; gm.q_lo = q.lo; gm.k_hi = k.hi; gm.k_lo = k.lo;
                    gm.swin_tokmap = tokmap[v]; gm.swin_logit_scale = h->V(w.logit_scale);
                    gm.swin_N = g.N; gm.swin_img_rows = (int)img_rows;
                    if (v_direct_ok && !no_fusion_v) {
                        gm.vt_hi = vt.hi; gm.vt_lo = vt.lo;
                        gm.swin_vtokmap = vtokmap[v]; gm.swin_img_velems = (int)img_velems;
                        if (!vt_zeroed && g.npadv != g.wa) {
                            CHK(hipMemsetAsync(vt.hi, 0, (size_t)p.B * img_velems * 2, c.s));
                            if (vt.lo) CHK(hipMemsetAsync(vt.lo, 0, (size_t)p.B * img_velems * 2, c.s));
                        }
                        vt_zeroed = true;
                    }
                }
                v_fused = gm.swin_vtokmap != nullptr;
                CHK(OPLC(mdpt_launch_gemm, gm, c.s));
            }
            if (!v_fused)
                CHK(OPLC(mdpt_launch_swin_qkv_prep, x, rowmap[v], h->V(w.logit_scale), q.hi, q.lo, k.hi, k.lo, vt.hi, vt.lo, p.B, g.N, g.nw, g.wa,
                                              g.npad, g.npadv, g.heads, c.s, !qk_fused));
            float* lut_l = (float*)(c.ws + p.sw.lut + (size_t)blk_index * p.sw.lut_stride);
            ++blk_index;
            {
                AttnParams a;
                memset(&a, 0, sizeof(a));
                a.q_hi = q.hi; a.q_lo = q.lo; a.k_hi = k.hi; a.k_lo = k.lo; a.vt_hi = vt.hi; a.vt_lo = vt.lo;
                a.out_hi = att.hi; a.out_lo = att.lo;
                a.B = p.B * g.nw; a.heads = g.heads; a.N = g.wa; a.npad = g.npad; a.npadv = g.npadv; a.F = F; a.x3 = h->x3c(CLS_ATTN);
                a.head_dim = 32; a.out_ld = Fp;
                a.bias_lut = lut_l; a.bias_elen = (2 * g.wh - 1) * (2 * g.ww - 1);
                a.tq = c.at<int>(p.sw.tq); a.tk = c.at<int>(p.sw.tk);
                a.win_nw = g.nw; a.rowmap = rowmap[v]; a.region = v ? region[1] : nullptr; a.region_ld = g.wa;
                a.bias_run4 = (g.ww % 4 == 0 && g.wa % 4 == 0) ? 1 : 0;
                a.bias_row = 2 * g.ww - 1; a.bias_ww = g.ww;  // conflict-free LDS image of the bias table (attention.hip)
                a.swin_ls = h->V(w.logit_scale);
#ifdef MDPT_DEBUG_SWITCHES  // A/B builds only
                static const bool no_run4 = getenv("MDPT_SWIN_NO_RUN4") != nullptr;
                if (no_run4) a.bias_run4 = 0;
#endif
                if (c.attn_dump && c.attn_dump[blk_index - 1]) CHK(OPLC(mdpt_launch_attn_weights, a, (float*)c.attn_dump[blk_index - 1], c.s));
                CHK(OPLC(mdpt_launch_attention, a, c.s));
            }
            {
                GemmParams gm = base_params(c, h->M(w.proj), att, rows, Fp);
                gm.bias = h->V(w.proj_b);
                gm.out_f32 = x; gm.ldc = F;
                CHK(wrc_bias(c, gm, h->M(w.proj), gm.bias, g.N, g.N));
                CHK(OPLC(mdpt_launch_gemm, gm, c.s));
            }
            CHK(OPLC(mdpt_launch_ln_res, x, resid, h->V(w.ln1_w), h->V(w.ln1_b), 1e-5f, resid, xn.hi, xn.lo, rows, F, c.s, Fp));
            {
                GemmParams gm = base_params(c, h->M(w.fc1), xn, rows, Fp);
                gm.bias = h->V(w.fc1_b);
                gm.act = MDPT_ACT_GELU;
                gm.out_hi = hb.hi; gm.out_lo = hb.lo; gm.ldc = 4 * F;
                CHK(wrc_bias(c, gm, h->M(w.fc1), gm.bias, g.N, g.N));
                CHK(OPLC(mdpt_launch_gemm, gm, c.s));
            }
            const float* fc2_part = nullptr;
            {
                GemmParams gm = base_params(c, h->M(w.fc2), hb, rows, 4 * F);
                gm.bias = h->V(w.fc2_b);
                gm.out_f32 = x; gm.ldc = F;
                CHK(wrc_bias(c, gm, h->M(w.fc2), gm.bias, g.N, g.N));
                // the late stages are few tiles of long K (stage 2 of SwinV2-L at batch 16: 108 8-phase tiles x 48 K tiles, which ran the lockstep
                // 128x128 tile at 0.25 of peak): K in two fixed ranges, twice the workgroups, and the post-norm that follows adds the second
                // range's partial sums. Decided by K alone (swin_ksplit) - at EVERY batch size, every tile form computes the
                // same two sums: an image's bits do not depend on its batch. The partial plane lives in the unused two thirds of the QKV-sized
                // fp32 buffer.
                if (swin_ksplit(F, gm.K)) {  // (a forced lockstep tile other than 64x64 has no split form: those launches run the 64x64 one)
                    gm.ksplit = 2; gm.ks_part = x + (size_t)rows * F;
                    fc2_part = gm.ks_part;
                }
                CHK(OPLC(mdpt_launch_gemm, gm, c.s));
            }
            CHK(OPLC(mdpt_launch_ln_res, x, resid, h->V(w.ln2_w), h->V(w.ln2_b), 1e-5f, resid, xn.hi, xn.lo, rows, F, c.s, Fp, fc2_part));
            if (c.block_dump && c.block_dump[blk_index - 1])  // block output tokens [B, N_s, F_s] (image_encoder_model.py:213-225)
                CHK(hipMemcpyAsync(c.block_dump[blk_index - 1], resid, (size_t)rows * F * 4, hipMemcpyDeviceToDevice, c.s));
            if (c.norm_wanted(blk_index - 1))  // per-token norms / one channel of the same tokens: fp32 [B, gh_s, gw_s]
                CHK(OPLC(mdpt_launch_row_norm, resid, c.norm_dump ? (float*)c.norm_dump[blk_index - 1] : nullptr,
                                             c.chan_dump ? (float*)c.chan_dump[blk_index - 1] : nullptr,
                                             c.chan_dump && c.chan_dump[blk_index - 1] ? c.chan_index[blk_index - 1] : 0, p.B, g.N, g.N, 0, F, c.s));
        }
        Planes tp = c.pl(p.tap[s]);
        CHK(OPLC(mdpt_launch_f32_to_planes, resid, tp.hi, tp.lo, (size_t)rows, F, Fp, c.s));
        if (taps_f32) CHK(hipMemcpyAsync(taps_f32[s], resid, (size_t)rows * F * 4, hipMemcpyDeviceToDevice, c.s));
        if (s < 3) {
            const auto& pm = h->w.merge[s];
            const int Fo = h->hid[s + 1], rows_o = rows / 4;
            CHK(OPLC(mdpt_launch_swin_merge_gather, resid, xn.hi, xn.lo, p.B, g.gh, g.gw, F, c.s));
            GemmParams gm = base_params(c, h->M(pm.reduction), xn, rows_o, 4 * F);
            gm.out_f32 = x; gm.ldc = Fo;
            CHK(wrc_bias(c, gm, h->M(pm.reduction), nullptr, g.N / 4, g.N / 4));
            CHK(OPLC(mdpt_launch_gemm, gm, c.s));
            CHK(OPLC(mdpt_launch_ln_res, x, nullptr, h->V(pm.norm_w), h->V(pm.norm_b), 1e-5f,
                                   c.at<float>(p.sw.resid[s + 1]), xn.hi, xn.lo, rows_o, Fo, c.s));
        }
    }
    return 0;
}

// tokens of stage s are already NHWC [B, gh_s, gw_s, F_s]: 3x3 conv (no bias) to the fusion width (reassembly_model.py:113-122)
int run_reassemble_swin(const Ctx& c) {
    const mdpt_handle* h = c.h;
    const Plan& p = c.p;
    for (int s = 0; s < 4; ++s) {
        const int sh = p.sw.g0h >> s, sw = p.sw.g0w >> s, F = h->hid[s];
        Planes rb = c.pl(p.r_bf[s]);
        GemmParams g = base_params(c, h->M(h->w.reasm[s].fuse_proj), c.pl(p.tap[s]), p.B * sh * sw, h->hidp[s]);
        as_conv(g, sh, sw, h->hidp[s], sh, sw, 1);
        g.out_f32 = c.at<float>(p.r_f32[s]);
        g.out_hi = rb.hi; g.out_lo = rb.lo; g.relu_bf16 = 1; g.ldc = h->Cp;
        CHK(OPLC(mdpt_launch_gemm, g, c.s));
    }
    return 0;
}
