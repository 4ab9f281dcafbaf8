// gemm.hip, part 5: the 8-phase 256x256x64 main loop (half-tile stager, body, kernel entry) and the rule that maps a generic launch to a direct epilogue.
template <int AMODE, bool F8 = false>
struct HalfStager {  // BM = BN = 256, 8 waves, BK = 64: chunk c = wave + 8 i covers rows 8c..8c+7; half h = chunks i in {2h, 2h+1}
    static constexpr int A_BYTES = 256 * 128;
    // Measured on one box, interleaved (profiles/r03_gemm8_staging_ab.txt): the buffered form is NOT faster for the dense GEMMs (QKV 240.7
    // vs 237.8 us, fc1 366.8 vs 364.0, residual GEMMs 231.5 vs 230.5) - their loop is bound by the 64 DMA instructions per K tile, not by
    // the 16 VALU operations of the pointer form - so the pointer form stays the default and -DMDPT_GEMM8_BUF_STAGING builds the other one.
#ifdef MDPT_GEMM8_BUF_STAGING
    static constexpr bool BUFFERED = AMODE != MDPT_A_CONV3;
#else
    static constexpr bool BUFFERED = false;
#endif
    // Dense / token rows (BUFFERED): LDS-DMA through buffer descriptors (buffer_load_dwordx4 ... offen lds) whose base is THIS tile's
    // first row: the per-lane byte offsets are constants of the tile (row, swizzled k-chunk), the position along K and the 64-row step
    // between a wave's DMA instructions are SCALAR offsets - no 64-bit pointer arithmetic in the loop (16 VALU operations per K tile in
    // the pointer form: measured 2500 -> 2200 cycles per K tile on the conv kernel that was written this way first) - and rows past
    // M / N fail the descriptor's bounds check and are staged as zeros (tools/probes/buffer_lds_oob.hip) instead of being clamped.
    // 3x3 taps (im2col-free conv): per-lane source pointers, recomputed per tap (global_load_lds).
    __amdgpu_buffer_rsrc_t rs_a, rs_w;
    unsigned a_voff[4], b_voff;
    int a_soff, b_soff, a_row_step, b_row_step;
    const op_t* a_base_hi; const op_t* a_base_lo; const op_t* w_base_hi; const op_t* w_base_lo;
    size_t a_bytes, w_bytes;
    const op_t* a_ptr[4];
    int a_pix[4], a_y[4], a_x[4], a_ko[4];
    const op_t* b_ptr[4];
    ptrdiff_t a_hi_minus_lo, w_lo_minus_hi;
    const op_t* conv_plane;
    int a_pass, a_k0, a_tap, a_ci, b_pass, b_k0;
    int st_m0, st_n0, b_step;
    bool a_f8, b_f8;  // GemmParams::f8: the pass being staged reads fp8 planes (128-element K tiles, byte planes: f8_cross.h)

    // GemmParams::f8: this wave's source pointers of pass `pass` (see Stager::place in gemm_common.inc)
    __device__ __forceinline__ void place_a(const GemmParams& p, int pass, int wave, int lane) {
        const int lrow = lane >> 3;
        a_f8 = pass < p.npass - 1;
        const char* Ab = a_f8 ? (const char*)p.A_lo + (pass == 1 ? p.a8_off : 0) : (const char*)p.A_hi;
        const int esz = a_f8 ? 1 : 2;
        conv_plane = (const op_t*)Ab;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = (wave + 8 * i) * 8 + lrow;
            int m = st_m0 + r;
            m = m < p.M ? m : p.M - 1;
            if (AMODE == MDPT_A_DENSE) {
                a_ptr[i] = (const op_t*)(Ab + (size_t)m * p.lda * esz) + a_ko[i];
            } else if (AMODE == MDPT_A_TOKENS) {
                const int b = m / p.tok_np, t = m - b * p.tok_np;
                a_ptr[i] = (const op_t*)(Ab + ((size_t)b * p.tok_stride + 1 + t) * p.lda * esz) + a_ko[i];
            }
        }
    }
    __device__ __forceinline__ void place_b(const GemmParams& p, int pass, int wave, int lane) {
        const int lrow = lane >> 3;
        b_f8 = pass < p.npass - 1;
        const char* Wb = b_f8 ? (const char*)(pass == 1 ? p.W8_lo : p.W8) : (const char*)p.W_hi;
        const int esz = b_f8 ? 1 : 2;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = (wave + 8 * i) * 8 + lrow;
            int n = st_n0 + r;
            n = n < p.N ? n : p.N - 1;
            b_ptr[i] = (const op_t*)(Wb + (size_t)n * p.K * esz) + a_ko[i];  // (the same rows / swizzle key as the A chunks; packed panels: row stride K)
        }
        // F8 kernels stage B through b_ptr[0] + i * b_step (rows 64 i further on, same swizzle key: the launcher sends only N % 256 == 0 here, no row
        // is clamped): three 64-bit pointers fewer in a kernel that carries two main loops at the 256-register limit (with four pointers the fp16
        // loop of the implicit-conv form reloaded spilled pointer pairs from scratch, a vmcnt(0) each: 370 us against 310 us for three fp16 passes)
        b_step = 64 * p.K * esz;
    }

    static __device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void* base, size_t bytes) {
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)(unsigned)(bytes < 0xFFFFFFF0ull ? bytes : 0xFFFFFFF0ull), 0x00020000);
    }

    __device__ __forceinline__ void init(const GemmParams& p, int m0, int n0, int wave, int lane) {
        const int lrow = lane >> 3, slot = lane & 7;
        const op_t* A0 = p.npass >= 2 ? p.A_lo : p.A_hi;  // two passes = A_lo*W_hi, A_hi*W_hi (the weights stay on their hi plane)
        a_pass = a_k0 = a_tap = a_ci = b_pass = b_k0 = 0;
        if constexpr (BUFFERED) {
            constexpr unsigned OOB = 0xFFFFFFF0u;
            const int rows_here = p.M - m0 < 256 ? p.M - m0 : 256, cols_here = p.N - n0 < 256 ? p.N - n0 : 256;
            // source row of logical row m (token rows skip the cls row of every image)
            auto src_row = [&](int m) -> size_t {
                if (AMODE == MDPT_A_TOKENS) { const int b = m / p.tok_np, t = m - b * p.tok_np; return (size_t)b * p.tok_stride + 1 + t; }
                return (size_t)m;
            };
            const size_t row0 = src_row(m0), row_last = src_row(m0 + rows_here - 1);
            a_base_hi = p.A_hi + row0 * p.lda; a_base_lo = p.npass >= 2 ? p.A_lo + row0 * p.lda : a_base_hi;
            a_bytes = (row_last - row0 + 1) * p.lda * 2;
            w_base_hi = p.W_hi + (size_t)n0 * p.ldw; w_base_lo = p.npass == 3 ? p.W_lo + (size_t)n0 * p.ldw : w_base_hi;
            w_bytes = ((size_t)(cols_here - 1) * p.ldw + p.K) * 2;
            rs_a = rsrc(p.npass >= 2 ? a_base_lo : a_base_hi, a_bytes);  // pass 0 of the multi-pass forms: A_lo * W_hi
            rs_w = rsrc(w_base_hi, w_bytes);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = (wave + 8 * i) * 8 + lrow;
                const int koff = (slot ^ ((r >> 1) & 7)) * 8;
                a_voff[i] = r < rows_here ? (unsigned)(((src_row(m0 + r) - row0) * p.lda + koff) * 2) : OOB;
            }
            {
                const int r = wave * 8 + lrow;  // rows of DMA instruction i: r + 64 i, same swizzle key
                b_voff = (unsigned)(((size_t)r * p.ldw + ((slot ^ ((r >> 1) & 7)) * 8)) * 2);
            }
            a_soff = b_soff = 0;
            b_row_step = 64 * p.ldw * 2;
            a_row_step = 0;
            a_hi_minus_lo = w_lo_minus_hi = 0;
            conv_plane = nullptr;
            return;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = (wave + 8 * i) * 8 + lrow;
            const int koff = (slot ^ ((r >> 1) & 7)) * 8;
            int m = m0 + r;
            m = m < p.M ? m : p.M - 1;
            a_ko[i] = koff;
            a_ptr[i] = nullptr;
            a_pix[i] = a_y[i] = a_x[i] = 0;
            if (AMODE == MDPT_A_DENSE) {
                a_ptr[i] = A0 + (size_t)m * p.lda + koff;
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
                if constexpr (F8) { a_y[i] = (a_y[i] << 16) | (x * p.cstride); a_x[i] = 0; }  // (maps of < 32768 rows / columns: the launcher's 32-bit plane checks imply it)
            }
            int n = n0 + r;
            n = n < p.N ? n : p.N - 1;
            b_ptr[i] = p.W_hi + (size_t)n * p.ldw + koff;
        }
        a_hi_minus_lo = p.npass >= 2 ? p.A_hi - p.A_lo : 0;
        w_lo_minus_hi = p.npass == 3 ? p.W_lo - p.W_hi : 0;
        conv_plane = A0;
        st_m0 = m0; st_n0 = n0; a_f8 = b_f8 = false;
        if constexpr (F8) { place_a(p, 0, wave, lane); place_b(p, 0, wave, lane); }
    }

    template <int H>
    __device__ __forceinline__ void issue_a(const GemmParams& p, char* buf, int wave) {
        typedef __attribute__((address_space(3))) void* lds_ptr_t;
        if constexpr (BUFFERED) {
#pragma unroll
            for (int i = 2 * H; i < 2 * H + 2; ++i)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_a, (lds_ptr_t)(buf + (wave + 8 * i) * 1024), 16, a_voff[i], a_soff, 0, 0);
            if (H == 1) {  // both halves of this K tile are on their way: advance K (and the bf16x3 operand planes at roll-over)
                a_soff += 128;
                if (a_soff == p.K * 2) {
                    a_soff = 0;
                    if (a_pass == 0) rs_a = rsrc(a_base_hi, a_bytes);  // passes 1, 2 read A_hi
                    ++a_pass;
                }
            }
            return;
        }
#pragma unroll
        for (int i = 2 * H; i < 2 * H + 2; ++i) {
            const op_t* src;
            if (AMODE == MDPT_A_CONV3) {
                const int ky = (a_tap * 11) >> 5, kx = a_tap - 3 * ky;
                const int iy = (F8 ? (a_y[i] >> 16) : a_y[i]) + ky, ix = (F8 ? (a_y[i] & 0xFFFF) - 1 : a_x[i]) + kx;  // (F8: y * stride - 1 and x * stride packed in one register)
                const bool ok = (unsigned)iy < (unsigned)p.Hi && (unsigned)ix < (unsigned)p.Wi;
                const size_t e = (size_t)(a_pix[i] + iy * p.Wi + ix) * p.Cin + a_ci;  // element = byte offset in an fp8 plane (even: Cin % 128 == 0)
                src = ok ? conv_plane + ((F8 && a_f8) ? (e >> 1) : e) + a_ko[i] : p.zero_page + a_ko[i];
            } else {
                src = a_ptr[i];
                a_ptr[i] += 64;
            }
            glds16(src, buf + (wave + 8 * i) * 1024);
        }
        if (F8 && H == 1 && a_f8) {  // an fp8 K tile: 128 elements, one tap of a 128-channel block
            a_k0 += 128;
            if (AMODE == MDPT_A_CONV3) { if (++a_tap == 9) { a_tap = 0; a_ci += 128; } }
            if (a_k0 == p.K) {
                a_k0 = 0; a_tap = 0; a_ci = 0;
                ++a_pass;
                place_a(p, a_pass, wave, threadIdx.x & 63);
            }
        } else
        if (H == 1) {  // both halves of this K tile are on their way: advance K (and the bf16x3 operand planes at roll-over)
            a_k0 += 64;
            if (AMODE == MDPT_A_CONV3) {
                if (++a_tap == 9) { a_tap = 0; a_ci += 64; }  // tap-inner K order (see Stager)
            }
            if (a_k0 == p.K) {
                a_k0 = 0; a_tap = 0; a_ci = 0;
                const ptrdiff_t da = (a_pass == 0 ? a_hi_minus_lo : 0) - p.K;
                if (a_pass == 0) conv_plane = p.A_hi;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (AMODE != MDPT_A_CONV3) a_ptr[i] += da;
                ++a_pass;
            }
        }
    }

    template <int H>
    __device__ __forceinline__ void issue_b(const GemmParams& p, char* buf, int wave) {
        typedef __attribute__((address_space(3))) void* lds_ptr_t;
        if constexpr (BUFFERED) {
#pragma unroll
            for (int i = 2 * H; i < 2 * H + 2; ++i)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (lds_ptr_t)(buf + A_BYTES + (wave + 8 * i) * 1024), 16, b_voff, b_soff + i * b_row_step, 0, 0);
            if (H == 1) {
                b_soff += 128;
                if (b_soff == p.K * 2) {  // bf16x3 passes: W_hi, W_lo, W_hi
                    b_soff = 0;
                    rs_w = rsrc(b_pass == 0 ? w_base_lo : w_base_hi, w_bytes);
                    ++b_pass;
                }
            }
            return;
        }
        if constexpr (F8) {
#pragma unroll
            for (int i = 2 * H; i < 2 * H + 2; ++i) glds16((const op_t*)((const char*)b_ptr[0] + i * b_step), buf + A_BYTES + (wave + 8 * i) * 1024);
            if (H == 1) b_ptr[0] += 64;
        } else {
#pragma unroll
        for (int i = 2 * H; i < 2 * H + 2; ++i) {
            glds16(b_ptr[i], buf + A_BYTES + (wave + 8 * i) * 1024);
            b_ptr[i] += 64;
        }
        }
        if (F8 && H == 1 && b_f8) {
            b_k0 += 128;
            if (b_k0 == p.K) {
                b_k0 = 0;
                ++b_pass;
                place_b(p, b_pass, wave, threadIdx.x & 63);
            }
        } else
        if (H == 1) {
            b_k0 += 64;
            if (b_k0 == p.K) {
                b_k0 = 0;
                const ptrdiff_t dw = (b_pass == 0 ? w_lo_minus_hi : -w_lo_minus_hi) - p.K;
#pragma unroll
                for (int i = 0; i < 4; ++i) b_ptr[i] += dw;
                ++b_pass;
            }
        }
    }
};

// FAST (dense rows, one pass - every encoder GEMM of the bf16 mode): operand staging without ANY per-K-tile state. A phase's MFMA block is
// 16 x 16 = 256 cycles and the other wave group's whole load phase has to fit under it, so every instruction of a load phase is on the
// critical path (profiles/r03_gemm8_loop_experiments.txt: ~10 scalar instructions + 4 branches per K tile cost 7 %). Here the operands go
// through buffer descriptors over this tile's rows (LDS-DMA, buffer_load ... lds): ONE per-lane byte offset per operand for the whole
// kernel, the K position and the 64-row step between a wave's DMA instructions are scalar offsets computed from the loop counter, rows past
// M / N fail the bounds check and are staged as zeros, and the last iteration (which issues nothing) is peeled off the loop instead of
// being tested for in every phase.
// F8 (fp16 build): GemmParams::f8 - the first T8 K tiles are fp8 tiles of the cross-term passes (f8_cross.h): the same staging, the same
// fragment reads (a lane's two 16-byte reads are the 32 operand bytes of one 16x16x128 MFMA), 8 block-scaled MFMAs per phase instead of 16.
template <int AMODE, int EKIND, bool SW, bool RI = false, bool FAST = false, bool F8 = false>
__device__ __forceinline__ void gemm8_body(const GemmParams& p, char* smem, const int dmode, const int m0, const int n0,
                                           const unsigned long long t_start) {
    static_assert(!RI || SW, "residual-initialised accumulators use the swapped operand order (4 consecutive columns per lane)");
    static_assert(!F8 || (!FAST && !RI && MDPT_HAVE_F8), "fp8 cross terms: state-machine stager, fp16 build");
    static_assert(!FAST || AMODE == MDPT_A_DENSE, "the stateless staging is for dense rows");
    constexpr int A_BYTES = 256 * 128, BUF = 2 * A_BYTES;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2, wc = wave & 3;
    unsigned long long t_first = 0, t_loop = 0;
    constexpr bool swapped = SW;
    HalfStager<AMODE, F8> st;
    if constexpr (!FAST) st.init(p, m0, n0, wave, lane);
    typedef __attribute__((address_space(3))) void* lds_ptr_t;
    __amdgpu_buffer_rsrc_t rs_a, rs_w;
    unsigned fa_voff = 0, fb_voff = 0;
    int fa_step = 0, fb_step = 0;
    if constexpr (FAST) {
        const int rows_here = p.M - m0 < 256 ? p.M - m0 : 256, cols_here = p.N - n0 < 256 ? p.N - n0 : 256;
        rs_a = tile_rsrc(p.A_hi + (size_t)m0 * p.lda, (size_t)rows_here * p.lda * 2);
        rs_w = tile_rsrc(p.W_hi + (size_t)n0 * p.ldw, ((size_t)(cols_here - 1) * p.ldw + p.K) * 2);
        const int r = wave * 8 + (lane >> 3);  // DMA instruction i of this wave stages rows r + 64 i (same swizzle key for all four)
        const int koff = ((lane & 7) ^ ((r >> 1) & 7)) * 8;
        fa_voff = (unsigned)(r * p.lda + koff) * 2u;
        fb_voff = (unsigned)(r * p.ldw + koff) * 2u;
        fa_step = 64 * p.lda * 2;
        fb_step = 64 * p.ldw * 2;
    }
    // half-tile H of the K tile at byte offset KB_ (FAST) / of the stager's next K tile (state machine) -> ring buffer BUF_
#define ISSUE_A(H_, BUF_, KB_)                                                                                          \
    do {                                                                                                                \
        if constexpr (FAST) {                                                                                           \
            _Pragma("unroll") for (int i = 2 * (H_); i < 2 * (H_) + 2; ++i)                                             \
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_a, (lds_ptr_t)((BUF_) + (wave + 8 * i) * 1024), 16, fa_voff, (KB_) + i * fa_step, 0, 0); \
        } else {                                                                                                        \
            st.template issue_a<H_>(p, BUF_, wave);                                                                     \
        }                                                                                                               \
    } while (0)
#define ISSUE_B(H_, BUF_, KB_)                                                                                          \
    do {                                                                                                                \
        if constexpr (FAST) {                                                                                           \
            _Pragma("unroll") for (int i = 2 * (H_); i < 2 * (H_) + 2; ++i)                                             \
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (lds_ptr_t)((BUF_) + 256 * 128 + (wave + 8 * i) * 1024), 16, fb_voff, (KB_) + i * fb_step, 0, 0); \
        } else {                                                                                                        \
            st.template issue_b<H_>(p, BUF_, wave);                                                                     \
        }                                                                                                               \
    } while (0)

    // fragment read offsets (16x16x32 MFMA: lane = (row l&15, 16-byte k-chunk l>>4)); key(row) = (row >> 1) & 7 as staged
    const int l15 = lane & 15, lh = lane >> 4, key = (l15 >> 1) & 7;
    const int a_off0 = (grp * 64 + l15) * 128 + ((lh ^ key) << 4), a_off1 = (grp * 64 + l15) * 128 + (((4 + lh) ^ key) << 4);
    const int b_off0 = A_BYTES + (wc * 32 + l15) * 128 + ((lh ^ key) << 4), b_off1 = A_BYTES + (wc * 32 + l15) * 128 + (((4 + lh) ^ key) << 4);

    f32x4 acc[2][2][4][2];
    if constexpr (!RI) {
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[a][b][i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }

    opx8 fa[4][2], fb0[2][2], fb1[2][2];
#define LOAD_A(QM_, BUF_)                                                                                             \
    do {                                                                                                              \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                               \
            fa[i][0] = *(const opx8*)(smem + (BUF_) * BUF + (QM_) * 16384 + i * 2048 + a_off0);                      \
            fa[i][1] = *(const opx8*)(smem + (BUF_) * BUF + (QM_) * 16384 + i * 2048 + a_off1);                      \
        }                                                                                                             \
    } while (0)
#define LOAD_B(DST_, QN_, BUF_)                                                                                       \
    do {                                                                                                              \
        _Pragma("unroll") for (int j = 0; j < 2; ++j) {                                                               \
            DST_[j][0] = *(const opx8*)(smem + (BUF_) * BUF + (QN_) * 16384 + j * 2048 + b_off0);                    \
            DST_[j][1] = *(const opx8*)(smem + (BUF_) * BUF + (QN_) * 16384 + j * 2048 + b_off1);                    \
        }                                                                                                             \
    } while (0)
#define MFMA_Q(QM_, QN_, FB_)                                                                                         \
    do {                                                                                                              \
        __builtin_amdgcn_s_setprio(1);                                                                                \
        _Pragma("unroll") for (int kk = 0; kk < 2; ++kk)                                                              \
            _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                             \
                _Pragma("unroll") for (int j = 0; j < 2; ++j)                                                         \
                    acc[QM_][QN_][i][j] = swapped ? MDPT_MFMA_16x16x32(FB_[j][kk], fa[i][kk], acc[QM_][QN_][i][j], 0, 0, 0) \
                                                  : MDPT_MFMA_16x16x32(fa[i][kk], FB_[j][kk], acc[QM_][QN_][i][j], 0, 0, 0); \
        __builtin_amdgcn_s_setprio(0);                                                                                \
    } while (0)
#if MDPT_HAVE_F8
    // E8M0 scales of the weight rows this lane's four 16-column blocks read: byte 2 qn + j = row n0 + 128 qn + 32 wc + 16 j + l15
    int wsc = 0, wsc_lo = 0;
    const int asc = F8_A_SCALE;  // the activations' constant E8M0 scale (a VGPR operand of every scaled MFMA)
    if constexpr (F8) {
#pragma unroll
        for (int b4 = 0; b4 < 4; ++b4) {
            int n = n0 + (b4 >> 1) * 128 + wc * 32 + (b4 & 1) * 16 + l15;
            n = n < p.N ? n : p.N - 1;
            wsc |= (int)p.S8[n] << (8 * b4);
            if (p.npass == 3) wsc_lo |= (int)p.S8_lo[n] << (8 * b4);
        }
    }
#define MFMA_Q8_ONE(QM_, QN_, FB_, I_, J_, WS_)                                                                       \
    do {                                                                                                              \
        if constexpr (swapped) f8_mfma16_w_first<2 * (QN_) + (J_)>(acc[QM_][QN_][I_][J_], f8_cat(FB_[J_][0], FB_[J_][1]), f8_cat(fa[I_][0], fa[I_][1]), WS_, asc); \
        else f8_mfma16_a_first<2 * (QN_) + (J_)>(acc[QM_][QN_][I_][J_], f8_cat(fa[I_][0], fa[I_][1]), f8_cat(FB_[J_][0], FB_[J_][1]), asc, WS_); \
    } while (0)
#define MFMA_Q8(QM_, QN_, FB_, WS_)                                                                                   \
    do {                                                                                                              \
        __builtin_amdgcn_s_setprio(1);                                                                                \
        MFMA_Q8_ONE(QM_, QN_, FB_, 0, 0, WS_); MFMA_Q8_ONE(QM_, QN_, FB_, 0, 1, WS_);                                 \
        MFMA_Q8_ONE(QM_, QN_, FB_, 1, 0, WS_); MFMA_Q8_ONE(QM_, QN_, FB_, 1, 1, WS_);                                 \
        MFMA_Q8_ONE(QM_, QN_, FB_, 2, 0, WS_); MFMA_Q8_ONE(QM_, QN_, FB_, 2, 1, WS_);                                 \
        MFMA_Q8_ONE(QM_, QN_, FB_, 3, 0, WS_); MFMA_Q8_ONE(QM_, QN_, FB_, 3, 1, WS_);                                 \
        __builtin_amdgcn_s_setprio(0);                                                                                \
    } while (0)
#endif
// RI form: quadrant (QM_, QN_)'s residual loads (inline asm, in-order return) have landed once at most N_ younger vector-memory operations
// are outstanding; naming the eight accumulators as read-write operands keeps every use of them below this statement
#define ACC_READY(QM_, QN_, N_)                                                                                                          \
    asm volatile("s_waitcnt vmcnt(" #N_ ")"                                                                                              \
                 : "+v"(acc[QM_][QN_][0][0]), "+v"(acc[QM_][QN_][0][1]), "+v"(acc[QM_][QN_][1][0]), "+v"(acc[QM_][QN_][1][1]),           \
                   "+v"(acc[QM_][QN_][2][0]), "+v"(acc[QM_][QN_][2][1]), "+v"(acc[QM_][QN_][3][0]), "+v"(acc[QM_][QN_][3][1])            \
                 :                                                                                                                       \
                 : "memory")

    // ---- prologue: K tiles 0 and 1 complete (even / odd buffer); T >= 2 and even (checked by the launcher)
    const int T = F8 ? ktiles_total(p, p.K) : (p.K / 64) * p.npass;
    const int T8 = F8 ? ktiles_f8(p, p.K) : 0, T8a = F8 ? p.K / 128 : 0;  // fp8 tiles of all cross-term passes / of the first one (both even: launcher)
    char* const bufE = smem;
    char* const bufO = smem + BUF;
    ISSUE_A(0, bufE, 0);
    ISSUE_B(0, bufE, 0);
    ISSUE_B(1, bufE, 0);
    ISSUE_A(1, bufE, 0);
    if constexpr (RI) {
        // Accumulators start at the residual tile (out = resid + A W^T + bias, in place): 32 x 16-byte loads per lane in the order the
        // quadrants are first used (P1 (0,0), P2 (0,1), P3 (1,1), P4 (1,0)), issued between the DMAs of K tile 0 and K tile 1. vmcnt retires
        // in order, so the first MFMA block waits for K tile 0 + quadrant (0,0) only; the other 24 loads land under the first phases (counted
        // waits in front of each quadrant's first MFMA in the first iteration, ACC_READY). Lanes outside the tile read 0.
        // The loads are inline asm: beside LDS-DMA hipcc waits vmcnt(0) for any register load it knows about (the whole prologue would
        // drain before the first MFMA); an asm load is invisible to its wait insertion and is waited for by hand (ACC_READY below,
        // which also names the destination registers so that nothing reads them earlier).
        constexpr unsigned OOB = 0xFFFFFFF0u;
        typedef __attribute__((ext_vector_type(4))) int i32x4;
        const int rows_here = p.M - m0 < 256 ? p.M - m0 : 256;
        const unsigned long long base = (unsigned long long)(p.resid + (size_t)m0 * p.ldr);
        i32x4 rs;  // raw buffer descriptor of this tile's rows: base, stride 0, num_records = bytes, dst_sel/format word as tile_rsrc()
        rs[0] = __builtin_amdgcn_readfirstlane((int)(unsigned)base);
        rs[1] = __builtin_amdgcn_readfirstlane((int)(unsigned)(base >> 32) & 0xFFFF);
        rs[2] = __builtin_amdgcn_readfirstlane((int)(unsigned)((size_t)rows_here * p.ldr * 4));
        rs[3] = 0x00020000;
        const unsigned row_b = (unsigned)p.ldr * 4u;
        auto load_quadrant = [&](int qm, int qn) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int nc = n0 + qn * 128 + wc * 32 + j * 16 + 4 * lh;
                const unsigned col = nc < p.N ? (unsigned)nc * 4u : OOB;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const unsigned row = (unsigned)(qm * 128 + grp * 64 + i * 16 + l15) * row_b;
                    const unsigned off = col == OOB ? OOB : row + col;
                    asm volatile("s_nop 4\n\tbuffer_load_dwordx4 %0, %1, %2, 0 offen" : "=v"(acc[qm][qn][i][j]) : "v"(off), "s"(rs) : "memory");
                }
            }
        };
        load_quadrant(0, 0);
        ISSUE_B(0, bufO, 128);
        ISSUE_A(0, bufO, 128);
        ISSUE_B(1, bufO, 128);
        ISSUE_A(1, bufO, 128);
        load_quadrant(0, 1);
        load_quadrant(1, 1);
        load_quadrant(1, 0);
        WAIT_VM(40);  // K tile 0 has landed: 8 (quadrant (0,0)) + 8 (K tile 1) + 24 younger operations may still be in flight
    } else {
        ISSUE_B(0, bufO, 128);
        ISSUE_A(0, bufO, 128);
        ISSUE_B(1, bufO, 128);
        ISSUE_A(1, bufO, 128);
        WAIT_VM(8);
    }
    BAR();
    if (p.dbg_times) t_first = memtime_now();
    if (grp == 1) BAR();  // stagger: group 1 runs one barrier behind group 0


    // fp16 build, GemmParams::wscale: the packed planes carry a power-of-two factor s, so the residual enters the accumulators as resid * s (exact;
    // the epilogue multiplies by 1 / s). One wave-uniform test per quadrant of the FIRST iteration; the bf16 build compiles nothing here.
    const float ri_scale = (MDPT_OP_IS_F16 && RI && p.wscale) ? p.wscale[0] : 1.0f;
#define SCALE_Q(QM_, QN_)                                                                                             \
    do {                                                                                                              \
        if (MDPT_OP_IS_F16 && RI && ri_scale != 1.0f) {                                                               \
            _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                             \
                _Pragma("unroll") for (int j = 0; j < 2; ++j) acc[QM_][QN_][i][j] *= ri_scale;                        \
        }                                                                                                             \
    } while (0)
#define GEMM8_ITER(MORE_, FIRST_, MQ)                                                                                       \
    do {                                                                                                              \
        const int kE = t * 128 + 256, kO = kE + 128; /* byte offsets of K tiles t + 2 / t + 3 (FAST staging) */        \
        /* P1 */                                                                                                      \
        LOAD_B(fb0, 0, 0); PIN(); LOAD_A(0, 0); PIN();                                                                \
        WAIT_LGKM(8); BAR(); WAIT_LGKM(0); PIN();                                                                     \
        if (FIRST_) { ACC_READY(0, 0, 32); SCALE_Q(0, 0); PIN(); } /* younger: 8 (K tile 1) + 24 */                    \
        MQ(0, 0, fb0); BAR();                                                                                     \
        /* P2 */                                                                                                      \
        LOAD_B(fb1, 1, 0); PIN();                                                                                     \
        if (MORE_) ISSUE_B(0, bufE, kE);                                                             \
        BAR(); WAIT_LGKM(0); PIN();                                                                                   \
        if (FIRST_) { ACC_READY(0, 1, 18); SCALE_Q(0, 1); PIN(); } /* younger: 16 + 2 */                              \
        MQ(0, 1, fb1); BAR();                                                                                     \
        /* P3 */                                                                                                      \
        LOAD_A(1, 0); PIN();                                                                                          \
        if (MORE_) ISSUE_A(0, bufE, kE);                                                             \
        PIN(); WAIT_LGKM(0); BAR(); PIN();                                                                            \
        if (FIRST_) { ACC_READY(1, 1, 12); SCALE_Q(1, 1); PIN(); } /* younger: 8 + 4 */                               \
        MQ(1, 1, fb1); BAR();                                                                                     \
        /* P4 */                                                                                                      \
        if (MORE_) { ISSUE_B(1, bufE, kE); ISSUE_A(1, bufE, kE); PIN(); WAIT_VM(8); } else { WAIT_VM(0); }                      \
        BAR();                                                                                                        \
        if (FIRST_) { ACC_READY(1, 0, 8); SCALE_Q(1, 0); PIN(); } /* the phase's own vmcnt(8) already covers the last 8 loads */ \
        MQ(1, 0, fb0); BAR();                                                                                     \
        /* P5 */                                                                                                      \
        LOAD_B(fb0, 0, 1); PIN(); LOAD_A(0, 1); PIN();                                                                \
        WAIT_LGKM(8); BAR(); WAIT_LGKM(0); PIN();                                                                     \
        MQ(0, 0, fb0); BAR();                                                                                     \
        /* P6 */                                                                                                      \
        LOAD_B(fb1, 1, 1); PIN();                                                                                     \
        if (MORE_) ISSUE_B(0, bufO, kO);                                                             \
        BAR(); WAIT_LGKM(0); PIN();                                                                                   \
        MQ(0, 1, fb1); BAR();                                                                                     \
        /* P7 */                                                                                                      \
        LOAD_A(1, 1); PIN();                                                                                          \
        if (MORE_) ISSUE_A(0, bufO, kO);                                                             \
        PIN(); WAIT_LGKM(0); BAR(); PIN();                                                                            \
        MQ(1, 1, fb1); BAR();                                                                                     \
        /* P8 */                                                                                                      \
        if (MORE_) { ISSUE_B(1, bufO, kO); ISSUE_A(1, bufO, kO); PIN(); WAIT_VM(8); }                                          \
        BAR();                                                                                                        \
        MQ(1, 0, fb0); BAR();                                                                                     \
    } while (0)
    // RI: the residual loads are waited for in the first iteration only (t == 0: T >= 4 is checked by the launcher, so that iteration's
    // DMA issues all happen and the younger-operation counts of ACC_READY are exact); the accumulators stay in the loop-carried registers
    if constexpr (FAST) {
        // compile-time MORE / FIRST: the first iteration (RI: counted waits for the residual loads) and the last one (issues nothing,
        // drains) are peeled; T >= 4 when RI (launcher)
        int t = 0;
        if constexpr (RI) {
            GEMM8_ITER(true, true, MFMA_Q);
            t = 2;
        }
        for (; t + 2 < T; t += 2) GEMM8_ITER(true, false, MFMA_Q);
        GEMM8_ITER(false, false, MFMA_Q);
    } else {
        int t = 0;
#if MDPT_HAVE_F8
        if constexpr (F8) {  // the cross-term passes on fp8 tiles (always followed by the fp16 pass: more = true)
#define MQ8A(QM_, QN_, FB_) MFMA_Q8(QM_, QN_, FB_, wsc)
#define MQ8B(QM_, QN_, FB_) MFMA_Q8(QM_, QN_, FB_, wsc_lo)
            for (; t < T8a; t += 2) GEMM8_ITER(true, false, MQ8A);
            for (; t < T8; t += 2) GEMM8_ITER(true, false, MQ8B);
#undef MQ8A
#undef MQ8B
        }
#endif
        for (; t < T; t += 2) {
            const bool more = t + 2 < T;  // wave-uniform: the last iteration issues nothing after P1 and drains at P4
            GEMM8_ITER(more, (RI && t == 0), MFMA_Q);
        }
    }
#undef GEMM8_ITER
#undef SCALE_Q
#undef ACC_READY
#undef ISSUE_A
#undef ISSUE_B
    if (grp == 0) BAR();  // re-join the two groups
#undef LOAD_A
#undef LOAD_B
#undef MFMA_Q
#if MDPT_HAVE_F8
#undef MFMA_Q8
#undef MFMA_Q8_ONE
#endif
    if (p.dbg_times) t_loop = memtime_now();
    if constexpr (SW) {
        if (EKIND == MDPT_E_SWQKV) {
            if (dmode == DM_F32) {  // V columns as fp32 rows (swin_v_prep follows)
                if (HAVE_IMGB && p.bias_img_stride) epilogue_direct<DM_F32, false, MDPT_ACT_NONE, HAVE_IMGB>(p, acc, m0, n0, grp, wc, lane);
                else epilogue_direct<DM_F32, false, MDPT_ACT_NONE>(p, acc, m0, n0, grp, wc, lane);
            } else if (HAVE_IMGB && p.bias_img_stride) {
                if (p.q_lo) epilogue_swin_qk<true, HAVE_IMGB>(p, acc, m0, n0, grp, wc, lane);
                else epilogue_swin_qk<false, HAVE_IMGB>(p, acc, m0, n0, grp, wc, lane);
            } else if (p.q_lo) {
                epilogue_swin_qk<true>(p, acc, m0, n0, grp, wc, lane);
            } else {
                epilogue_swin_qk<false>(p, acc, m0, n0, grp, wc, lane);
            }
        } else if (EKIND == MDPT_E_QKV) {
            if (HAVE_IMGB && p.bias_img_stride) {
                if (p.q_lo) epilogue_direct<DM_QK, true, MDPT_ACT_NONE, HAVE_IMGB>(p, acc, m0, n0, grp, wc, lane);
                else epilogue_direct<DM_QK, false, MDPT_ACT_NONE, HAVE_IMGB>(p, acc, m0, n0, grp, wc, lane);
            } else if (p.q_lo) epilogue_direct<DM_QK, true, MDPT_ACT_NONE>(p, acc, m0, n0, grp, wc, lane);
            else epilogue_direct<DM_QK, false, MDPT_ACT_NONE>(p, acc, m0, n0, grp, wc, lane);
        } else if (HAVE_IMGB && dmode == DM_BF16 && p.bias_img_stride) {  // the encoder's fc1 with a per-image bias table (single plane or hi + lo)
            if (p.act == MDPT_ACT_GELU) {
                if (p.out_lo) epilogue_direct<DM_BF16, true, MDPT_ACT_GELU, HAVE_IMGB>(p, acc, m0, n0, grp, wc, lane);
                else epilogue_direct<DM_BF16, false, MDPT_ACT_GELU, HAVE_IMGB>(p, acc, m0, n0, grp, wc, lane);
            } else {
                if (p.out_lo) epilogue_direct<DM_BF16, true, MDPT_ACT_NONE, HAVE_IMGB>(p, acc, m0, n0, grp, wc, lane);
                else epilogue_direct<DM_BF16, false, MDPT_ACT_NONE, HAVE_IMGB>(p, acc, m0, n0, grp, wc, lane);
            }
        } else if (dmode == DM_BF16) {
            const int sel = (p.out_lo ? 3 : 0) + (p.act == MDPT_ACT_GELU ? 2 : (p.act == MDPT_ACT_RELU || p.relu_bf16) ? 1 : 0);
            switch (sel) {
                case 0: epilogue_direct<DM_BF16, false, MDPT_ACT_NONE>(p, acc, m0, n0, grp, wc, lane); break;
                case 1: epilogue_direct<DM_BF16, false, MDPT_ACT_RELU>(p, acc, m0, n0, grp, wc, lane); break;
                case 2: epilogue_direct<DM_BF16, false, MDPT_ACT_GELU>(p, acc, m0, n0, grp, wc, lane); break;
                case 3: epilogue_direct<DM_BF16, true, MDPT_ACT_NONE>(p, acc, m0, n0, grp, wc, lane); break;
                case 4: epilogue_direct<DM_BF16, true, MDPT_ACT_RELU>(p, acc, m0, n0, grp, wc, lane); break;
                default: epilogue_direct<DM_BF16, true, MDPT_ACT_GELU>(p, acc, m0, n0, grp, wc, lane); break;
            }
        } else if (dmode == DM_F32 || dmode == DM_RINIT) {  // DM_RINIT: the residual is already in the accumulators
            if (HAVE_IMGB && p.bias_img_stride) epilogue_direct<DM_F32, false, MDPT_ACT_NONE, HAVE_IMGB>(p, acc, m0, n0, grp, wc, lane);
            else epilogue_direct<DM_F32, false, MDPT_ACT_NONE>(p, acc, m0, n0, grp, wc, lane);
        } else {
            epilogue_direct<DM_RESID, false, MDPT_ACT_NONE>(p, acc, m0, n0, grp, wc, lane);
        }
        if (p.dbg_times && tid == 0) {
            const unsigned long long t_issued = memtime_now();  // all of this wave's stores issued, none waited for
            stamp_record(p.dbg_times, t_start, t_first, t_loop, STAMP_HW_ID, t_issued);
        }
        return;
    }
    if ((EKIND == MDPT_E_QKV && dmode == DM_VT) || (EKIND == MDPT_E_SWQKV && dmode == DM_SWVT)) {
        if (EKIND == MDPT_E_SWQKV) {
            if (HAVE_IMGB && p.bias_img_stride) {
                if (p.vt_lo) epilogue_swin_vt<true, HAVE_IMGB>(p, acc, m0, n0, grp, wc, lane);
                else epilogue_swin_vt<false, HAVE_IMGB>(p, acc, m0, n0, grp, wc, lane);
            } else if (p.vt_lo) epilogue_swin_vt<true>(p, acc, m0, n0, grp, wc, lane);
            else epilogue_swin_vt<false>(p, acc, m0, n0, grp, wc, lane);
        } else if (HAVE_IMGB && p.bias_img_stride) {
            if (p.vt_lo) epilogue_direct_vt<true, HAVE_IMGB>(p, acc, m0, n0, grp, wc, lane);
            else epilogue_direct_vt<false, HAVE_IMGB>(p, acc, m0, n0, grp, wc, lane);
        } else if (p.vt_lo) {
            epilogue_direct_vt<true>(p, acc, m0, n0, grp, wc, lane);
        } else {
            epilogue_direct_vt<false>(p, acc, m0, n0, grp, wc, lane);
        }
        if (p.dbg_times && tid == 0) stamp_record(p.dbg_times, t_start, t_first, t_loop, STAMP_NO_ID);
        return;
    }
    __syncthreads();  // every wave is done reading the ring: reuse it as epilogue staging

    // ---- epilogue: per quadrant two [32][32] blocks through the wave-private strip (C layout of the 16x16 MFMA:
    //      acc[r] = C[4*(lane>>4) + r][lane&15])
    float* strip = (float*)smem + wave * (32 * 32);
#pragma unroll
    for (int qm = 0; qm < 2; ++qm)
#pragma unroll
        for (int qn = 0; qn < 2; ++qn)
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) {
#pragma unroll
                for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int r = 0; r < 4; ++r) strip[(ii * 16 + 4 * lh + r) * 32 + j * 16 + l15] = acc[qm][qn][rb * 2 + ii][j][r];
                epilogue_block<32, EKIND>(p, strip, lane, m0 + qm * 128 + grp * 64 + rb * 32, n0 + qn * 128 + wc * 32);
            }
    if (p.dbg_times && tid == 0) stamp_record(p.dbg_times, t_start, t_first, t_loop, 4);
}

// Operand order of the MFMAs: swapped -> accumulators hold 4 consecutive COLUMNS per lane and one of the direct epilogues
// applies; plain order (4 consecutive ROWS per lane) + LDS strip for every other epilogue. For the generic epilogue the choice is
// a property of the launch and is made on the host (DMODE template parameter: one main loop + one epilogue per kernel keeps the
// register allocation of the 256-VGPR loop predictable); QKV launches decide per tile (tiles that contain V columns are written
// transposed, token-contiguous, through the strip).
__host__ __device__ inline int generic_direct_mode(const GemmParams& p) {
    // a per-image bias table needs the IMGB epilogues (fp16 build, >= 256 rows per image, the forms the encoder uses)
    const bool imgb_ok = HAVE_IMGB && p.bias_img_rows >= 256 && p.bias && !p.gamma && !p.relu_bf16 && p.act != MDPT_ACT_RELU;
    const bool plain = !p.up_src && (!p.bias_img_stride || imgb_ok);
    const bool fits = (size_t)256 * p.ldc * 4 < 0xFFFFFFF0ull;  // tile-local byte offsets of the buffer ops are 32-bit
    // relu_bf16 without an fp32 copy is just a ReLU activation (first conv of every residual conv unit)
    if (plain && fits && p.out_hi && !p.out_f32 && !p.gamma && !p.resid && !(p.relu_bf16 && p.act != MDPT_ACT_NONE)) return DM_BF16;
    if (plain && fits && !p.bias_img_stride && p.out_f32 && !p.out_hi && p.gamma && p.resid && p.resid == p.out_f32 && p.bias && p.act == MDPT_ACT_NONE && p.ldr == p.ldc)
        return DM_RESID;
    if (plain && fits && p.acc_init && p.out_f32 && !p.out_hi && !p.gamma && p.resid == p.out_f32 && p.ldr == p.ldc && p.act == MDPT_ACT_NONE && !p.relu_bf16)
        return DM_RINIT;
    if (plain && fits && p.out_f32 && !p.out_hi && !p.gamma && !p.resid && p.act == MDPT_ACT_NONE && !p.relu_bf16) return DM_F32;
    return DM_NONE;
}

// F8: the launch runs its cross-term passes on fp8 planes (GemmParams::f8) - a kernel of its own, so that the kernels of every other launch
// keep the register allocation they were tuned with
template <int AMODE, int EKIND, int DMODE, bool F8 = false>
__global__ __launch_bounds__(512, 1) void gemm8_kernel(const GemmParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned long long t_start = 0;
    if (p.dbg_times) t_start = memtime_now();
    int m0, n0;
    tile_coords((p.N + 255) / 256, 256, 256, m0, n0);
    if constexpr (EKIND == MDPT_E_SWQKV) {
        // SwinV2 QKV projection (the host guarantees dense A, 2F % 256 == 0 and 32-bit plane offsets): Q / K tiles -> DM_SWQK; V tiles ->
        // transposed window operand (DM_SWVT, plain operand order) when token runs of 4 stay together, else fp32 rows for swin_v_prep
        const bool fast = p.npass == 1;
        if (n0 >= 2 * p.F && p.swin_vtokmap) {
            if (fast) gemm8_body<AMODE, EKIND, false, false, true>(p, smem, DM_SWVT, m0, n0, t_start);
            else gemm8_body<AMODE, EKIND, false>(p, smem, DM_SWVT, m0, n0, t_start);
        } else {
            const int dm = n0 >= 2 * p.F ? DM_F32 : DM_SWQK;
            if (fast) gemm8_body<AMODE, EKIND, true, false, true>(p, smem, dm, m0, n0, t_start);
            else gemm8_body<AMODE, EKIND, true>(p, smem, dm, m0, n0, t_start);
        }
    } else if (EKIND == MDPT_E_QKV) {
        // per tile: Q / K columns only -> swapped order + head-major direct epilogue; V columns only -> plain order + transposed
        // direct epilogue; a tile that straddles 2F (odd head counts) or planes beyond 32-bit offsets -> plain order + LDS strip
#ifdef MDPT_GEMM8_NO_FAST
        const bool fast = false;
#else
        const bool fast = AMODE == MDPT_A_DENSE && p.npass == 1;  // bf16 mode: stateless operand staging
#endif
        if (n0 + 256 <= 2 * p.F && (size_t)p.M * p.F * 2 < 0xFFFFFFF0ull) {
            if constexpr (AMODE == MDPT_A_DENSE) {
                if (fast) gemm8_body<AMODE, EKIND, true, false, true>(p, smem, DM_QK, m0, n0, t_start);
                else gemm8_body<AMODE, EKIND, true>(p, smem, DM_QK, m0, n0, t_start);
            } else {
                gemm8_body<AMODE, EKIND, true>(p, smem, DM_QK, m0, n0, t_start);
            }
        } else if (n0 >= 2 * p.F && n0 + 256 <= p.N && (size_t)(p.M / p.npad) * p.F * p.npadv * 2 < 0xFFFFFFF0ull) {
            if constexpr (AMODE == MDPT_A_DENSE) {
                if (fast) gemm8_body<AMODE, EKIND, false, false, true>(p, smem, DM_VT, m0, n0, t_start);
                else gemm8_body<AMODE, EKIND, false>(p, smem, DM_VT, m0, n0, t_start);
            } else {
                gemm8_body<AMODE, EKIND, false>(p, smem, DM_VT, m0, n0, t_start);
            }
        } else {
            gemm8_body<AMODE, EKIND, false>(p, smem, DM_NONE, m0, n0, t_start);
        }
    } else if constexpr (AMODE == MDPT_A_DENSE && DMODE == DM_F32) {
        // plain fp32 outputs; with GemmParams::ksplit > 1 (grid.y = range) this workgroup walks K range z of rows that are ldw wide: range 0 is the
        // normal kernel on a shorter K, ranges z >= 1 store bare partial sums (no bias) to the partial planes
        if constexpr (F8) {  // (no K split with fp8 cross terms: mdpt_launch_gemm)
            gemm8_body<AMODE, EKIND, true, false, false, true>(p, smem, DMODE, m0, n0, t_start);
            return;
        }
        GemmParams q = p;
        if (p.ksplit > 1) {
            const int z = (int)blockIdx.y, ks = p.K / p.ksplit;
            q.K = ks;
            q.A_hi = p.A_hi + z * ks; q.W_hi = p.W_hi + z * ks;
            if (p.npass >= 2) q.A_lo = p.A_lo + z * ks;
            if (p.npass == 3) q.W_lo = p.W_lo + z * ks;
            if (z > 0) { q.bias = nullptr; q.bias_img_stride = 0; q.out_f32 = p.ks_part + (size_t)(z - 1) * p.M * p.ldc; }
        }
        if (q.npass == 1) gemm8_body<AMODE, EKIND, true, false, true>(q, smem, DMODE, m0, n0, t_start);
        else gemm8_body<AMODE, EKIND, true, false, false>(q, smem, DMODE, m0, n0, t_start);
    } else if constexpr (AMODE == MDPT_A_DENSE && DMODE != DM_NONE) {
        // the encoder's hot forms: stateless staging when there is one pass (bf16 mode), the state-machine stager for bf16x3
#ifdef MDPT_GEMM8_NO_FAST  // A/B builds only
        if (false) {}
#else
        if (p.npass == 1) gemm8_body<AMODE, EKIND, true, DMODE == DM_RINIT, true>(p, smem, DMODE, m0, n0, t_start);
#endif
        else if constexpr (F8) gemm8_body<AMODE, EKIND, true, false, false, true>(p, smem, DMODE, m0, n0, t_start);
        else gemm8_body<AMODE, EKIND, true, DMODE == DM_RINIT, false>(p, smem, DMODE, m0, n0, t_start);
    } else {
        if constexpr (F8) gemm8_body<AMODE, EKIND, DMODE != DM_NONE, false, false, true>(p, smem, DMODE, m0, n0, t_start);
        else gemm8_body<AMODE, EKIND, DMODE != DM_NONE, DMODE == DM_RINIT>(p, smem, DMODE, m0, n0, t_start);
    }
}
