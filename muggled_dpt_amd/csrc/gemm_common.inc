// gemm.hip, part 1 (textually included inside its anonymous namespace, behind mfma_common.inc): the erf-GELU, hi / lo plane stores, the operand
// stager of the lockstep kernels and the XCD-aware tile map.
// Exact-GELU 0.5 v (1 + erf(v/sqrt2)) (reference: nn.GELU() default, components/misc_helpers.py:113).
// erf(|v|/sqrt2) = 1 - 2^(-|v| q(|v|)): -log2 erfc(|v|/sqrt2) = |v| q(|v|) with q a degree-7 polynomial (weighted minimax fit on
// |v| <= 5.8, where erfc reaches 7e-9; beyond it the positive leading coefficient keeps the exponent growing, an overflowing q gives
// 2^-inf = 0, no NaN from a finite v). |error of erf| <= 1e-7 in fp32 (tests/test_gelu_poly_cpu.py restates this arithmetic in numpy
// against scipy's erf); round 2-5's Abramowitz-Stegun 7.1.26 form read 5e-7 and needed TWO quarter-rate transcendentals per value
// (rcp and exp2) - the fc1 epilogue is VALU-bound and exposed (one workgroup per CU: nothing runs under it), this form needs one exp2
// and eight packed multiply-adds: 11.5 instead of 16 issue slots per value.
// The file is compiled with fp-contraction off (so that no template instantiation fuses differently from another); the multiply-adds
// of this function are EXPLICIT fmas - the same bits in every instantiation.
#define MDPT_GELU_Q0 1.1511051654815674f
#define MDPT_GELU_Q1 0.4592081904411316f
#define MDPT_GELU_Q2 0.052496179938316345f
#define MDPT_GELU_Q3 -0.00706342002376914f
#define MDPT_GELU_Q4 0.00013693643268197775f
#define MDPT_GELU_Q5 0.00018618021567817777f
#define MDPT_GELU_Q6 -3.93776863347739e-05f
#define MDPT_GELU_Q7 2.8349124931992264e-06f
__device__ __forceinline__ float gelu_erf(float v) {
    const float a = fabsf(v);
    float q = MDPT_GELU_Q7;
    q = __builtin_fmaf(q, a, MDPT_GELU_Q6);
    q = __builtin_fmaf(q, a, MDPT_GELU_Q5);
    q = __builtin_fmaf(q, a, MDPT_GELU_Q4);
    q = __builtin_fmaf(q, a, MDPT_GELU_Q3);
    q = __builtin_fmaf(q, a, MDPT_GELU_Q2);
    q = __builtin_fmaf(q, a, MDPT_GELU_Q1);
    q = __builtin_fmaf(q, a, MDPT_GELU_Q0);
    const float erf_abs = 1.0f - __builtin_amdgcn_exp2f(-(q * a));
    const float h = 0.5f * v;
    return __builtin_fmaf(h, copysignf(erf_abs, v), h);
}

// The same function on PAIRS of values: every multiply / fma becomes one packed instruction (v_pk_mul_f32 / v_pk_fma_f32: two lanes of
// IEEE fp32, the same bits as the scalar form above), only the exp2 stays scalar.
typedef f32x2 gelu_f32x2;
__device__ __forceinline__ gelu_f32x2 gelu_erf2(gelu_f32x2 v) {
    const gelu_f32x2 a = {fabsf(v[0]), fabsf(v[1])};
    gelu_f32x2 q = {MDPT_GELU_Q7, MDPT_GELU_Q7};
    q = __builtin_elementwise_fma(q, a, gelu_f32x2{MDPT_GELU_Q6, MDPT_GELU_Q6});
    q = __builtin_elementwise_fma(q, a, gelu_f32x2{MDPT_GELU_Q5, MDPT_GELU_Q5});
    q = __builtin_elementwise_fma(q, a, gelu_f32x2{MDPT_GELU_Q4, MDPT_GELU_Q4});
    q = __builtin_elementwise_fma(q, a, gelu_f32x2{MDPT_GELU_Q3, MDPT_GELU_Q3});
    q = __builtin_elementwise_fma(q, a, gelu_f32x2{MDPT_GELU_Q2, MDPT_GELU_Q2});
    q = __builtin_elementwise_fma(q, a, gelu_f32x2{MDPT_GELU_Q1, MDPT_GELU_Q1});
    q = __builtin_elementwise_fma(q, a, gelu_f32x2{MDPT_GELU_Q0, MDPT_GELU_Q0});
    const gelu_f32x2 arg = -(q * a);
    const gelu_f32x2 erf_abs = gelu_f32x2{1.0f, 1.0f} - gelu_f32x2{__builtin_amdgcn_exp2f(arg[0]), __builtin_amdgcn_exp2f(arg[1])};
    const gelu_f32x2 h = v * 0.5f;
    const gelu_f32x2 sgn = {copysignf(erf_abs[0], v[0]), copysignf(erf_abs[1], v[1])};
    return __builtin_elementwise_fma(h, sgn, h);
}

// lo_f8 / lo_a8: the lo plane in the fp8 form an F8 consumer reads (GemmParams::out_f8 / out_a8, f8_cross.h)
__device__ __forceinline__ void split_store4(op_t* hi, op_t* lo, size_t off, f32x4 v, size_t lo_f8 = 0, int lo_a8 = 0) {
    opx4 h;
#pragma unroll
    for (int e = 0; e < 4; ++e) h[e] = to_op(v[e]);
    *(opx4*)(hi + off) = h;
    if (lo) lo_store4(lo, off, lo_f8, lo_a8, v, h);
}

__device__ __forceinline__ void split_store8(op_t* hi, op_t* lo, size_t off, f32x4 v0, f32x4 v1, size_t lo_f8 = 0, int lo_a8 = 0) {
    opx8 h;
#pragma unroll
    for (int e = 0; e < 4; ++e) { h[e] = to_op(v0[e]); h[e + 4] = to_op(v1[e]); }
    *(opx8*)(hi + off) = h;
    if (lo) lo_store8(lo, off, lo_f8, lo_a8, v0, v1, h);
}

// K tiles of a launch: fp16 tiles are 64 elements; with GemmParams::f8 the npass - 1 cross-term passes come first on 128-element fp8 tiles
// (f8_cross.h) - the same 128 bytes per row either way. ktiles_f8 = how many of the tiles are fp8 tiles.
__host__ __device__ inline int ktiles_f8(const GemmParams& p, int kspan) { return p.f8 ? (kspan / 128) * (p.npass - 1) : 0; }
__host__ __device__ inline int ktiles_total(const GemmParams& p, int kspan) { return p.f8 ? ktiles_f8(p, kspan) + kspan / 64 : (kspan / 64) * p.npass; }

// ------------------------------------------------------------------------------------------------------------
// Operand stager: per-lane source addresses of this wave's LDS-DMA chunks for one (BM+BN) x BK slab, and the
// state machine that walks K (dense/token rows: a running pointer; 3x3 conv: tap / channel counters) and the
// bf16x3 operand planes.
// A DMA chunk (one global_load_lds_dwordx4 wave instruction, 1 KiB) is RPC rows x ROWB bytes; the lane feeds LDS
// row (chunk*RPC + lane/CPR), 16-B slot (lane%CPR), which must hold global chunk (slot ^ key(row)) with
// key(row) = (row / RPB) & (CPR-1): 16 consecutive rows then cover the 16 slots of a 256-B LDS bank row, so the
// ds_read_b128 fragment pattern (16 rows x 16 B per service group) is conflict-free.
// ------------------------------------------------------------------------------------------------------------
template <int BM, int BN, int NW, int BK, int AMODE, bool F8 = false>
struct Stager {
    static constexpr int ROWB = BK * 2, CPR = BK / 8, RPC = 64 / CPR, RPB = 256 / ROWB;
    static constexpr int CA = BM / RPC / NW, CB = BN / RPC / NW, NLOAD = CA + CB;
    static constexpr int A_BYTES = BM * ROWB, B_BYTES = BN * ROWB, SLAB = A_BYTES + B_BYTES;
    static_assert(BM % (RPC * NW) == 0 && BN % (RPC * NW) == 0, "chunk split");

    const op_t* a_ptr[CA];
    int a_pix[CA], a_y[CA], a_x[CA], a_ko[CA];
    const op_t* b_ptr[CB];
    ptrdiff_t a_hi_minus_lo, w_lo_minus_hi;
    const op_t* conv_plane;
    int st_pass, st_k0, st_tap, st_ci, st_sub;  // conv K order: 64-channel block (st_ci) outer, tap, then the BK-wide part of the block (st_sub)
    int kspan;                                  // K extent this workgroup walks per pass (p.K, or p.K / ksplit from kofs on: GemmParams::ksplit)
    int st_tap0, st_ci0;                        // conv state at the start of the range
    int st_m0, st_n0;                           // (GemmParams::f8: the planes of a pass are re-placed from the tile origin at every pass switch)
    bool st_f8;                                 // the pass being staged reads fp8 planes: 128-element K tiles, byte planes (f8_cross.h)

    // GemmParams::f8: source pointers of pass `pass` for this wave's DMA chunks. Passes 0 .. npass - 2 read the fp8 planes (A: the e5m2 residue
    // plane, then the e5m2 plane of the values; W: e4m3 of W_hi, then of W - W_hi), the last pass the fp16 hi planes. Pointers stay op_t*: an
    // fp8 K tile is the same 128 bytes per row as an fp16 one, only the row stride (lda BYTES instead of lda elements) and the plane differ.
    __device__ __forceinline__ void place(const GemmParams& p, int pass, int wave, int lane) {
        const int lrow = lane / CPR, slot = lane % CPR;
        st_f8 = pass < p.npass - 1;
        const char* Ab = st_f8 ? (const char*)p.A_lo + (pass == 1 ? p.a8_off : 0) : (const char*)p.A_hi;
        const char* Wb = st_f8 ? (const char*)(pass == 1 ? p.W8_lo : p.W8) : (const char*)p.W_hi;
        const int esz = st_f8 ? 1 : 2;
        conv_plane = (const op_t*)Ab;
#pragma unroll
        for (int i = 0; i < CA; ++i) {
            const int r = (wave + NW * i) * RPC + lrow;
            int m = st_m0 + r;
            m = m < p.M ? m : p.M - 1;
            if (AMODE == MDPT_A_DENSE) {
                a_ptr[i] = (const op_t*)(Ab + (size_t)m * p.lda * esz) + a_ko[i];
            } else if (AMODE == MDPT_A_TOKENS) {
                const int b = m / p.tok_np, t = m - b * p.tok_np;
                a_ptr[i] = (const op_t*)(Ab + ((size_t)b * p.tok_stride + 1 + t) * p.lda * esz) + a_ko[i];
            }
        }
#pragma unroll
        for (int i = 0; i < CB; ++i) {
            const int r = (wave + NW * i) * RPC + lrow;
            const int koff = (slot ^ ((r / RPB) & (CPR - 1))) * 8;
            int n = st_n0 + r;
            n = n < p.N ? n : p.N - 1;
            b_ptr[i] = (const op_t*)(Wb + (size_t)n * p.K * esz) + koff;  // (f8: packed panels only, row stride K)
        }
    }

    __device__ __forceinline__ void init(const GemmParams& p, int m0, int n0, int wave, int lane, int kofs = 0, int kspan_ = 0) {
        kspan = kspan_ > 0 ? kspan_ : p.K;
        const int lrow = lane / CPR, slot = lane % CPR;
        const op_t* A0 = p.npass >= 2 ? p.A_lo : p.A_hi;  // operand plane of pass 0
#pragma unroll
        for (int i = 0; i < CA; ++i) {
            const int r = (wave + NW * i) * RPC + lrow;
            const int koff = (slot ^ ((r / RPB) & (CPR - 1))) * 8;
            int m = m0 + r;
            m = m < p.M ? m : p.M - 1;  // clamp: rows past M are computed and discarded
            a_pix[i] = a_y[i] = a_x[i] = 0;
            a_ko[i] = koff;
            a_ptr[i] = nullptr;
            if (AMODE == MDPT_A_DENSE) {
                a_ptr[i] = A0 + (size_t)m * p.lda + koff + kofs;
            } else if (AMODE == MDPT_A_TOKENS) {
                const int b = m / p.tok_np, t = m - b * p.tok_np;
                a_ptr[i] = A0 + ((size_t)b * p.tok_stride + 1 + t) * p.lda + koff;
            } else {
                const int hw = p.Ho * p.Wo;
                const int b = m / hw, rem = m - b * hw;
                const int y = rem / p.Wo, x = rem - y * p.Wo;
                a_pix[i] = b * p.Hi * p.Wi;
                a_y[i] = y * p.cstride - 1;
                a_x[i] = x * p.cstride - 1;
            }
        }
#pragma unroll
        for (int i = 0; i < CB; ++i) {
            const int r = (wave + NW * i) * RPC + lrow;
            const int koff = (slot ^ ((r / RPB) & (CPR - 1))) * 8;
            int n = n0 + r;
            n = n < p.N ? n : p.N - 1;
            b_ptr[i] = p.W_hi + (size_t)n * p.ldw + koff + kofs;
        }
        // plane switches at pass roll-over (three passes: A_lo*W_hi, A_hi*W_lo, A_hi*W_hi; two passes - the activation-split form -
        // A_lo*W_hi, A_hi*W_hi: the weights stay on their hi plane); all wave-uniform
        a_hi_minus_lo = p.npass >= 2 ? p.A_hi - p.A_lo : 0;
        w_lo_minus_hi = p.npass == 3 ? p.W_lo - p.W_hi : 0;
        conv_plane = A0;
        st_pass = st_k0 = st_sub = 0;
        // a K range that starts at kofs (a multiple of 64): conv K order k = (cb * 9 + tap) * 64 + c
        st_tap0 = AMODE == MDPT_A_CONV3 ? (kofs >> 6) % 9 : 0;
        st_ci0 = AMODE == MDPT_A_CONV3 ? ((kofs >> 6) / 9) * 64 : 0;
        st_tap = st_tap0; st_ci = st_ci0;
        st_m0 = m0; st_n0 = n0; st_f8 = false;
        if constexpr (F8) place(p, 0, wave, lane);  // (the launcher refuses f8 with a K split or a 32-wide K tile)
    }

    // issue this wave's NLOAD LDS-DMA instructions for the next slab into the ring slot at `slab_base`, then advance
    __device__ __forceinline__ void issue(const GemmParams& p, char* slab_base, int wave) {
        char* sA = slab_base;
        char* sB = slab_base + A_BYTES;
#pragma unroll
        for (int i = 0; i < CA; ++i) {
            const op_t* src;
            if (AMODE == MDPT_A_CONV3) {
                const int ky = (st_tap * 11) >> 5, kx = st_tap - 3 * ky;
                const int iy = a_y[i] + ky, ix = a_x[i] + kx;
                const bool ok = (unsigned)iy < (unsigned)p.Hi && (unsigned)ix < (unsigned)p.Wi;
                const size_t e = (size_t)(a_pix[i] + iy * p.Wi + ix) * p.Cin + st_ci + st_sub;  // element = byte offset in an fp8 plane (even: Cin % 128 == 0)
                src = ok ? conv_plane + ((F8 && st_f8) ? (e >> 1) : e) + a_ko[i] : p.zero_page + a_ko[i];
            } else {
                src = a_ptr[i];
                a_ptr[i] += BK;
            }
            glds16(src, sA + (wave + NW * i) * 1024);
        }
#pragma unroll
        for (int i = 0; i < CB; ++i) {
            glds16(b_ptr[i], sB + (wave + NW * i) * 1024);
            b_ptr[i] += BK;
        }
        if (F8 && st_f8) {  // an fp8 K tile: 128 elements, one tap of a 128-channel block
            st_k0 += 128;
            if (AMODE == MDPT_A_CONV3) { if (++st_tap == 9) { st_tap = 0; st_ci += 128; } }
            if (st_k0 == kspan) {
                st_k0 = 0; st_tap = 0; st_ci = 0; st_sub = 0;
                ++st_pass;
                place(p, st_pass, wave, threadIdx.x & 63);
            }
            return;
        }
        st_k0 += BK;
        if (AMODE == MDPT_A_CONV3) {  // k = (cb * 9 + tap) * 64 + c: the nine taps of a 64-channel block are consecutive K tiles
            st_sub += BK;
            if (st_sub == 64) {
                st_sub = 0;
                if (++st_tap == 9) { st_tap = 0; st_ci += 64; }
            }
        }
        if (st_k0 == kspan) {  // next pass: rewind K and switch operand planes
            st_k0 = 0; st_tap = st_tap0; st_ci = st_ci0; st_sub = 0;
            const ptrdiff_t da = (st_pass == 0 ? a_hi_minus_lo : 0) - kspan;
            const ptrdiff_t dw = (st_pass == 0 ? w_lo_minus_hi : -w_lo_minus_hi) - kspan;
            if (st_pass == 0) conv_plane = p.A_hi;
#pragma unroll
            for (int i = 0; i < CA; ++i)
                if (AMODE != MDPT_A_CONV3) a_ptr[i] += da;
#pragma unroll
            for (int i = 0; i < CB; ++i) b_ptr[i] += dw;
            ++st_pass;
        }
    }
};

// XCD-aware tile mapping (bijective for any grid size): the dispatcher places block b on XCD b%8; give every XCD a
// contiguous run of tiles (same A rows, all N tiles) so operand panels stay in that XCD's L2.
__device__ __forceinline__ void tile_coords(int tiles_n, int BM, int BN, int& m0, int& n0) {
    const int nwg = gridDim.x, swz = xcd_tile();
    if (tiles_n >= 8 && (tiles_n & 3) == 0) {
        // wide outputs (fc1: 16 column tiles, QKV: 12): row-major order makes the 32 concurrent tiles of an XCD cover 2 row
        // blocks x ALL columns, i.e. the whole weight matrix (8 MB for fc1, twice the 4 MB L2) is re-streamed for every pair
        // of row blocks (measured 969 MB fetched per fc1 launch vs 93 MB algorithmic). Walk 4-column panels instead: the
        // panel's weights (2 MB at K = 1024) stay in L2 while the row blocks stream past once per panel.
        const int tiles_m = nwg / tiles_n, per_panel = tiles_m * 4;
        const int panel = swz / per_panel, r = swz - panel * per_panel;
        m0 = (r >> 2) * BM;
        n0 = (panel * 4 + (r & 3)) * BN;
        return;
    }
    m0 = (swz / tiles_n) * BM;
    n0 = (swz % tiles_n) * BN;
}
