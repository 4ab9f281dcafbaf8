"""Every operand and epilogue form of mdpt_launch_gemm on its own operands (test hook mdpt_debug_gemm_form), in both operand formats, against the
float64 restatements of tests/gemm_forms_restate.py (proven on the CPU by tests/test_gemm_forms_cpu.py). `pytest -m gpu`.

Every output buffer is filled with a sentinel and has guard rows in front and behind; every byte a form does not own (guards, the cls / pad rows
of the patch output, the columns [npad, npadv) of Vt, planes a case does not pass) must come back bit-identical. Rows a gather must not read
(cls and pad rows of the token source) hold +-1e30.

Tiles requested per form, and the kernel the launcher's rules (gemm.hip resolve_tile / launch_tile / launch_pp) resolve them to. Tile values: 0 auto,
1 128x128, 2 256x256, 4 256x128 (32-wide K tiles), 6 64x64 - lockstep kernels, strip epilogues - and 5, the 8-phase 256x256 kernel:

  form                         0 (auto)        5 (8-phase) resolves to
  QKV  K = 128                 64x64           8-phase: Q / K tile direct (DM_QK), the V tile of F = 128 straddles N -> strip; F = 256: V tile direct (DM_VT);
                                               with a bias table: lockstep 256x256, except fp16 with >= 256 rows per image (npad 264): 8-phase IMGB epilogues
  QKV  K = 192 (3 K tiles)     64x64           lockstep 256x256 (odd K-tile count)
  PATCH K = 192 / 640          64x64           lockstep 256x256 / 8-phase + strip
  TOKENS K = 128               64x64           8-phase, buffered token rows, direct fp32 epilogue (DM_F32)
  D2S  K = 128                 64x64           8-phase + strip
  CONV3 stride 2, Cin 64 / 128 64x64           lockstep 256x256 (9 K tiles) / 8-phase conv stager, DM_F32
  HEAD                         the 128x32 kernel whatever is requested (one case, tile 0)
  ldw, bias table, npass       64x64           8-phase DM_F32 (bias table: fp16 with 264-row images IMGB direct, else lockstep strip epilogue
                                               via DM_NONE); npass 2 / 3: 8 / 12 K tiles, the state-machine stager
  K split                      64x64           8-phase DM_F32 ranges (N = 256, 8 or 4 K tiles per range); ks_all: 64x64 whatever is requested
  wscale + acc_init (fp16)     64x64           8-phase DM_RINIT (4 K tiles)
  tiles 1, 2, 4, 6 always run the lockstep kernel of that shape (64x64 with >= 32 K tiles: the 3-deep ring).

Tolerances. fp32 outputs against float64 of the same operands: 2e-5 max|ref| (the bound of tests/test_gpu_gemm_fuzz.py for the same loops). 16-bit
planes beside an fp32 output: hi = the format's round-to-nearest-even of that fp32 value, lo = the rounding of (value - hi), bit for bit. 16-bit
planes alone (Q, K, Vt, depth-to-space): |hi (+ lo) - ref| <= the fp32 bound + one ulp, where ulp(x) of a format with p stored significand bits and
smallest normal exponent emin is 2^(max(floor(log2 |x|), emin) - p): bf16 p = 7, emin = -126; fp16 p = 10, emin = -14 (rounding to nearest leaves
half an ulp; the fp32 error may carry a value over a rounding boundary, hence a whole one). With a lo plane the remainder hi + lo leaves is the
rounding of lo, and |lo| <= ulp(ref) / 2: one ulp of the format AT ulp(ref) / 2."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import gemm_forms_restate as rs

pytestmark = pytest.mark.gpu

SENT = 7.0
TILES = (0, 1, 2, 4, 5, 6)
INVALID = 1  # hipErrorInvalidValue: what mdpt_launch_gemm answers to a combination it refuses
DT_CODE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
# HEAD sigmoid (__expf): largest error against float64 measured on the MI355X over these cases (f32 output, pre-activations in [-6, 6]; Cin 64 /
# 128: 4.33e-7 / 5.95e-7 with bf16 operands, 4.85e-7 / 4.71e-7 with fp16), asserted at four times that (never above 1e-5 absolute on the [0, 1] output)
SIGMOID_MEASURED = 5.95e-7
SIGMOID_TOL = min(4 * SIGMOID_MEASURED, 1e-5)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from muggled_dpt_amd import native
    return native.load()


@pytest.fixture(params=["bf16", "fp16"])
def dt(request, lib):
    from muggled_dpt_amd import native
    request.addfinalizer(lambda: native.check(lib, lib.mdpt_debug_set_operand_format(0)))  # back to bf16 even when the test fails
    native.check(lib, lib.mdpt_debug_set_operand_format(1 if request.param == "fp16" else 0))
    return torch.float16 if request.param == "fp16" else torch.bfloat16


def rng(seed):
    return np.random.default_rng(seed)


def op(x, dtype):
    """float array -> device tensor rounded to the operand format"""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dtype).cuda()


def split(x, dtype):
    """hi / lo planes of fp32 values: hi = round(x), lo = round(x - hi) (csrc/dt_io.h round_dt, ew_common.inc plane stores)"""
    x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    hi = x.to(dtype)
    return hi.cuda(), (x - hi.float()).to(dtype).cuda()


def f32(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def f64(t):
    return t.detach().cpu().double().numpy()


class Out:
    """an output buffer: sentinel everywhere, three guard rows (rounded up to 16 bytes) in front and behind"""

    def __init__(self, shape, dtype):
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.g = (3 * self.shape[-1] + 7) // 8 * 8
        self.buf = torch.full((self.n + 2 * self.g,), SENT, device="cuda", dtype=dtype)
        self.ptr = self.buf.data_ptr() + self.g * self.buf.element_size()

    def get(self):
        return self.buf[self.g:self.g + self.n].reshape(self.shape).cpu()

    def guards_ok(self):
        return bool((self.buf[:self.g] == SENT).all()) and bool((self.buf[self.g + self.n:] == SENT).all())

    def untouched(self):
        return bool((self.buf == SENT).all())


def launch(lib, fn="mdpt_debug_gemm_form", **kw):
    from muggled_dpt_amd import native
    f = native.MdptGemmForm()
    for k, v in kw.items():
        if v is None:
            continue
        setattr(f, k, v.ptr if isinstance(v, Out) else (v.data_ptr() if torch.is_tensor(v) else v))
    rc = getattr(lib, fn)(ctypes.byref(f), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def ulp(x, dtype):
    p, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -140)))
    return 2.0 ** (np.maximum(e, emin) - p)


def bound32(ref):
    return 2e-5 * float(np.nanmax(np.abs(ref)))


def check_f32(out, ref, what):
    """fp32 output against float64; NaN in ref = not owned: must still hold the sentinel"""
    got = out.get().double().numpy()
    own = ~np.isnan(ref)
    err = float(np.abs(got[own] - ref[own]).max())
    assert err <= bound32(ref), f"{what}: max err {err:.3e} > {bound32(ref):.3e}"
    assert (got[~own] == SENT).all(), f"{what}: wrote elements it does not own"
    assert out.guards_ok(), f"{what}: wrote into the guard rows"


def check_planes(hi, lo, ref, dtype, what, extra=0.0):
    """16-bit planes without an fp32 copy against float64 (lo = None: the lo plane was not passed)"""
    got = hi.get().double().numpy() + (lo.get().double().numpy() if lo is not None else 0.0)
    own = ~np.isnan(ref)
    r = ref[own]
    tol = bound32(ref) + extra + (ulp(ulp(r, dtype) / 2, dtype) if lo is not None else ulp(r, dtype))
    over = np.abs(got[own] - r) - tol
    assert float(over.max()) <= 0.0, f"{what}: error exceeds the bound by {float(over.max()):.3e} (max err {float(np.abs(got[own] - r).max()):.3e})"
    for o in (hi, lo):
        if o is not None:
            assert (o.get().double().numpy()[~own] == SENT).all(), f"{what}: wrote elements it does not own"
            assert o.guards_ok(), f"{what}: wrote into the guard rows"


def check_split_of(hi, lo, v32, dtype, what, relu=False):
    """planes beside an fp32 output: the format's split of that fp32 value, bit for bit"""
    v = torch.relu(v32) if relu else v32
    h = v.to(dtype)
    assert torch.equal(hi.get(), h), f"{what}: hi plane is not the rounding of the fp32 output"
    if lo is not None:
        assert torch.equal(lo.get(), (v - h.float()).to(dtype)), f"{what}: lo plane is not the rounding of the remainder"
    assert hi.guards_ok() and (lo is None or lo.guards_ok()), f"{what}: wrote into the guard rows"


# ------------------------------------------------------------------------------------------------ QKV
@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("heads,npad,npadv,K", [(2, 40, 40, 128), (2, 40, 64, 128), (2, 264, 264, 128), (2, 40, 40, 192), (2, 40, 64, 192),
                                                (2, 264, 264, 192), (4, 264, 264, 128)])
def test_qkv_scatter(lib, dt, heads, npad, npadv, K, table, planes):
    from muggled_dpt_amd import native
    B, Fd = 3, heads * 64
    M, N = B * npad, 3 * Fd
    g = rng(heads * 1000 + npad + npadv + K)
    a, w = op(g.standard_normal((M, K)), dt), op(g.standard_normal((N, K)) / math.sqrt(K), dt)
    bias = g.standard_normal((B, N) if table else (N,)).astype(np.float32)
    q_ref, k_ref, vt_ref = rs.qkv(rs.product(f64(a), f64(w)), bias, B, npad, npadv, heads, 0.125, bias_img_rows=npad)
    bias_d = f32(bias)
    for tile in TILES:
        outs = {n: Out(s, dt) for n, s in (("q_hi", q_ref.shape), ("q_lo", q_ref.shape), ("k_hi", k_ref.shape), ("k_lo", k_ref.shape),
                                           ("vt_hi", vt_ref.shape), ("vt_lo", vt_ref.shape))}
        passed = {n: o for n, o in outs.items() if planes == 2 or n.endswith("_hi")}
        rc = launch(lib, a_hi=a, w_hi=w, M=M, N=N, K=K, lda=K, npass=1, amode=native.A_DENSE, ekind=native.E_QKV, tile=tile, bias=bias_d,
                    bias_img_stride=N if table else 0, bias_img_rows=npad if table else 0, F=Fd, heads=heads, npad=npad, npadv=npadv, qscale=0.125, **passed)
        assert rc == 0, lib.mdpt_last_error()
        what = f"QKV heads={heads} npad={npad} npadv={npadv} K={K} table={table} planes={planes} tile={tile}"
        for n, ref in (("q", q_ref), ("k", k_ref), ("vt", vt_ref)):
            check_planes(outs[n + "_hi"], outs[n + "_lo"] if planes == 2 else None, ref, dt, f"{what} {n}")
            if planes == 1:
                assert outs[n + "_lo"].untouched(), f"{what}: {n}_lo was not passed"


# ------------------------------------------------------------------------------------------------ PATCH
@pytest.mark.parametrize("with_pos", [True, False])
@pytest.mark.parametrize("K", [192, 640])
def test_patch_rows_behind_the_cls_row(lib, dt, K, with_pos):
    from muggled_dpt_amd import native
    B, tok_np, npad, N = 3, 25, 32, 128
    M = B * tok_np
    g = rng(K + with_pos)
    a, w = op(g.standard_normal((M, K)), dt), op(g.standard_normal((N, K)) / math.sqrt(K), dt)
    bias, pos = g.standard_normal(N).astype(np.float32), g.standard_normal((tok_np, N)).astype(np.float32)
    ref = rs.patch(rs.product(f64(a), f64(w)), bias, pos if with_pos else None, B, tok_np, npad)
    bias_d, pos_d = f32(bias), f32(pos)
    for tile in TILES:
        out = Out((B * npad, N), torch.float32)
        rc = launch(lib, a_hi=a, w_hi=w, M=M, N=N, K=K, lda=K, npass=1, amode=native.A_DENSE, ekind=native.E_PATCH, tile=tile, bias=bias_d,
                    pos=pos_d if with_pos else None, tok_np=tok_np, npad=npad, out_f32=out, ldc=N)
        assert rc == 0, lib.mdpt_last_error()
        check_f32(out, ref, f"PATCH K={K} pos={with_pos} tile={tile}")


# ------------------------------------------------------------------------------------------------ TOKENS
def test_token_rows_skip_cls_and_pad_rows(lib, dt):
    from muggled_dpt_amd import native
    B, tok_np, tok_stride, K, N = 3, 25, 32, 128, 64
    M = B * tok_np
    g = rng(11)
    src = g.standard_normal((B, tok_stride, K))
    big = 1e30 if dt == torch.bfloat16 else 6.0e4  # finite in the format (fp16 ends at 65504): a stray read destroys the result, no inf or NaN
    src[:, 0], src[:, 1 + tok_np:] = big, -big
    src[:, 1 + tok_np::2] = big
    a = op(src.reshape(B * tok_stride, K), dt)
    assert bool(torch.isfinite(a.float()).all())
    w, bias = op(g.standard_normal((N, K)) / math.sqrt(K), dt), g.standard_normal(N).astype(np.float32)
    ref = rs.generic(rs.product(rs.token_rows(f64(a), B, tok_np, tok_stride), f64(w)), bias)
    assert float(np.abs(ref).max()) < 100.0
    bias_d = f32(bias)
    for tile in TILES:
        out = Out((M, N), torch.float32)
        rc = launch(lib, a_hi=a, w_hi=w, M=M, N=N, K=K, lda=K, npass=1, amode=native.A_TOKENS, ekind=native.E_GENERIC, tile=tile, bias=bias_d,
                    tok_np=tok_np, tok_stride=tok_stride, out_f32=out, ldc=N, ldr=N)
        assert rc == 0, lib.mdpt_last_error()
        check_f32(out, ref, f"TOKENS tile={tile}")


# ------------------------------------------------------------------------------------------------ D2S
@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("cout", [64, 72])
@pytest.mark.parametrize("k", [2, 4])
def test_depth_to_space_scatter(lib, dt, k, cout, planes):
    from muggled_dpt_amd import native
    B, Ho, Wo, K = 2, 5, 7, 128
    M, N = B * Ho * Wo, k * k * cout
    g = rng(k * 100 + cout)
    a, w = op(g.standard_normal((M, K)), dt), op(g.standard_normal((N, K)) / math.sqrt(K), dt)
    bias = g.standard_normal(cout).astype(np.float32)
    ref = rs.d2s(rs.product(f64(a), f64(w)), bias, B, Ho, Wo, k, cout)
    bias_d = f32(bias)
    for tile in TILES:
        hi, lo = Out(ref.shape, dt), Out(ref.shape, dt)
        rc = launch(lib, a_hi=a, w_hi=w, M=M, N=N, K=K, lda=K, npass=1, amode=native.A_DENSE, ekind=native.E_D2S, tile=tile, bias=bias_d, Ho=Ho, Wo=Wo,
                    d2s_k=k, d2s_cout=cout, out_hi=hi, out_lo=lo if planes == 2 else None, ldc=N)
        assert rc == 0, lib.mdpt_last_error()
        check_planes(hi, lo if planes == 2 else None, ref, dt, f"D2S k={k} cout={cout} planes={planes} tile={tile}")
        assert planes == 2 or lo.untouched()


# ------------------------------------------------------------------------------------------------ HEAD
def _head_case(dt, cin):
    B, H, W = 2, 9, 11
    g = rng(cin)
    x = op(g.standard_normal((B, H, W, cin)), dt)
    w = op(rs.pack_conv3(g.standard_normal((32, cin, 3, 3)) / math.sqrt(9 * cin)), dt)
    bias = g.standard_normal(32).astype(np.float32) * 0.5
    acc = rs.product(rs.conv3_rows(f64(x), 1), f64(w))
    # positive 1x1 weights (no cancellation inside the sum), scaled so that the pre-activation spans 12, and a bias that centres the span: the
    # ReLU cuts the lower half of it, the sigmoid sees [-6, 6]
    u = g.uniform(0.1, 1.0, 32)
    s0 = np.maximum(acc + bias, 0.0) @ u
    head_w = (u * 12.0 / (s0.max() - s0.min())).astype(np.float32)
    s1 = np.maximum(acc + bias, 0.0) @ head_w.astype(np.float64)
    head_b = np.float32(-0.5 * float(s1.max() + s1.min()))
    return B, H, W, x, w, bias, head_w, head_b, acc


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("sigmoid", [False, True])
@pytest.mark.parametrize("cin", [64, 128])
def test_head_reduction_and_final_activation(lib, dt, cin, sigmoid, out_dtype):
    """Sigmoid through __expf: the largest error against float64 measured on the MI355X over the f32-output cases is 5.95e-7 (SIGMOID_MEASURED; every
    case prints its own figure); asserted at four times that, 2.38e-6."""
    from muggled_dpt_amd import native
    B, H, W, x, w, bias, head_w, head_b, acc = _head_case(dt, cin)
    M = B * H * W
    ref = rs.head(acc, bias, head_w, head_b, sigmoid)
    pre = np.maximum(acc + bias, 0.0) @ head_w.astype(np.float64) + float(head_b)
    assert -6.1 < pre.min() < -5.9 and 5.9 < pre.max() < 6.1 and 0.2 < float((pre < 0).mean()) < 0.8
    out = Out((M,), out_dtype)
    bias_d, hw_d, hb_d = f32(bias), f32(head_w), f32(np.array([head_b]))
    rc = launch(lib, a_hi=x, w_hi=w, M=M, N=32, K=9 * cin, lda=cin, npass=1, amode=native.A_CONV3, ekind=native.E_HEAD, tile=0, bias=bias_d, Hi=H, Wi=W,
                Cin=cin, Ho=H, Wo=W, cstride=1, head_w=hw_d, head_b=hb_d, head_sigmoid=int(sigmoid), head_out=out, head_out_dtype=DT_CODE[out_dtype])
    assert rc == 0, lib.mdpt_last_error()
    got = out.get().double().numpy()
    err = np.abs(got - ref)
    what = f"HEAD cin={cin} sigmoid={sigmoid} out={out_dtype}"
    print(f"{what} operands={dt}: max err {float(err.max()):.3e}")
    tol = SIGMOID_TOL if sigmoid else bound32(ref)
    if out_dtype != torch.float32:
        tol = tol + ulp(ref, out_dtype)
    assert float((err - tol).max()) <= 0.0, f"{what}: max err {float(err.max()):.3e}"
    assert out.guards_ok(), f"{what}: wrote into the guard rows"


# ------------------------------------------------------------------------------------------------ CONV3 stride 2
@pytest.mark.parametrize("cin", [64, 128])
@pytest.mark.parametrize("hw", [(9, 11), (8, 10)])
def test_conv3_stride_2_taps(lib, dt, hw, cin):
    from muggled_dpt_amd import native
    B, N = 2, 64
    Hi, Wi = hw
    Ho, Wo = -(-Hi // 2), -(-Wi // 2)
    M, K = B * Ho * Wo, 9 * cin
    g = rng(Hi * 10 + cin)
    x = op(g.standard_normal((B, Hi, Wi, cin)), dt)
    w = op(rs.pack_conv3(g.standard_normal((N, cin, 3, 3)) / math.sqrt(K)), dt)
    bias = g.standard_normal(N).astype(np.float32)
    ref = rs.generic(rs.product(rs.conv3_rows(f64(x), 2), f64(w)), bias)
    bias_d = f32(bias)
    first = None
    for tile in TILES:
        out = Out((M, N), torch.float32)
        rc = launch(lib, a_hi=x, w_hi=w, M=M, N=N, K=K, lda=cin, npass=1, amode=native.A_CONV3, ekind=native.E_GENERIC, tile=tile, bias=bias_d, Hi=Hi, Wi=Wi,
                    Cin=cin, Ho=Ho, Wo=Wo, cstride=2, out_f32=out, ldc=N, ldr=N)
        assert rc == 0, lib.mdpt_last_error()
        check_f32(out, ref, f"CONV3 stride 2 {Hi}x{Wi} cin={cin} tile={tile}")
        first = out.get() if first is None else first
        assert torch.equal(out.get(), first), f"CONV3 stride 2 {Hi}x{Wi} cin={cin}: tile {tile} differs from tile {TILES[0]} in bits"


# ------------------------------------------------------------------------------------------------ ldw
def test_k_range_of_wider_weight_rows(lib, dt):
    from muggled_dpt_amd import native
    M, N, K = 130, 256, 256
    g = rng(21)
    a, w2 = op(g.standard_normal((M, K)), dt), op(g.standard_normal((N, 2 * K)) / math.sqrt(K), dt)
    for half in (0, 1):
        packed = w2[:, half * K:(half + 1) * K].contiguous()
        ref = rs.product(f64(a), f64(packed))
        for tile in TILES:
            wide, narrow = Out((M, N), torch.float32), Out((M, N), torch.float32)
            common = dict(a_hi=a, M=M, N=N, K=K, lda=K, npass=1, amode=native.A_DENSE, ekind=native.E_GENERIC, tile=tile, ldc=N, ldr=N)
            assert launch(lib, w_hi=w2.data_ptr() + half * K * 2, ldw=2 * K, out_f32=wide, **common) == 0, lib.mdpt_last_error()
            assert launch(lib, w_hi=packed, ldw=0, out_f32=narrow, **common) == 0, lib.mdpt_last_error()
            check_f32(wide, ref, f"ldw = 2K, columns of half {half}, tile={tile}")
            check_f32(narrow, ref, f"packed half {half}, tile={tile}")
            assert torch.equal(wide.get(), narrow.get()), f"half {half} tile {tile}: the K range of wide rows differs in bits from the packed panel"


# ------------------------------------------------------------------------------------------------ per-image bias table, generic epilogue
@pytest.mark.parametrize("to_planes", [False, True])
@pytest.mark.parametrize("rows", [40, 264])
def test_generic_epilogue_with_a_bias_table(lib, dt, rows, to_planes):
    from muggled_dpt_amd import native
    B, N, K = 3, 256, 256
    M = B * rows
    g = rng(rows)
    a, w = op(g.standard_normal((M, K)), dt), op(g.standard_normal((N, K)) / math.sqrt(K), dt)
    table = g.standard_normal((B, N)).astype(np.float32)
    ref = rs.generic(rs.product(f64(a), f64(w)), table, rows)
    table_d = f32(table)
    for tile in TILES:
        o32, hi, lo = Out((M, N), torch.float32), Out((M, N), dt), Out((M, N), dt)
        rc = launch(lib, a_hi=a, w_hi=w, M=M, N=N, K=K, lda=K, npass=1, amode=native.A_DENSE, ekind=native.E_GENERIC, tile=tile, bias=table_d,
                    bias_img_stride=N, bias_img_rows=rows, ldc=N, ldr=N, **(dict(out_hi=hi, out_lo=lo) if to_planes else dict(out_f32=o32)))
        assert rc == 0, lib.mdpt_last_error()
        what = f"bias table rows={rows} planes={to_planes} tile={tile}"
        if to_planes:
            check_planes(hi, lo, ref, dt, what)
            assert o32.untouched(), what
        else:
            check_f32(o32, ref, what)
            assert hi.untouched() and lo.untouched(), what


# ------------------------------------------------------------------------------------------------ K split
@pytest.mark.parametrize("ksplit", [2, 4])
def test_k_split_range_0_and_partial_planes(lib, dt, ksplit):
    from muggled_dpt_amd import native
    M, N, K = 130, 256, 1024
    g = rng(ksplit)
    a, w = op(g.standard_normal((M, K)), dt), op(g.standard_normal((N, K)) / math.sqrt(K), dt)
    bias = g.standard_normal(N).astype(np.float32)
    planes_ref = rs.ksplit_planes(f64(a), f64(w), ksplit)
    ref = rs.generic(rs.product(f64(a), f64(w)), bias)
    bias_d = f32(bias)
    got = {}
    for tile in (native.TILE_64x64, native.TILE_PP256, native.TILE_AUTO):
        out, part = Out((M, N), torch.float32), Out((ksplit - 1, M, N), torch.float32)
        rc = launch(lib, a_hi=a, w_hi=w, M=M, N=N, K=K, lda=K, npass=1, amode=native.A_DENSE, ekind=native.E_GENERIC, tile=tile, bias=bias_d, out_f32=out,
                    ldc=N, ldr=N, ksplit=ksplit, ks_part=part)
        assert rc == 0, lib.mdpt_last_error()
        what = f"K split {ksplit} tile={tile}"
        check_f32(out, rs.generic(planes_ref[0], bias), f"{what} range 0")
        check_f32(part, np.stack(planes_ref[1:]), f"{what} partial planes")
        total = out.get()
        for z in range(ksplit - 1):  # the consumer's order: z = 1, 2, ...
            total = total + part.get()[z]
        err = float(np.abs(total.double().numpy() - ref).max())
        assert err <= bound32(ref), f"{what}: sum of the ranges, max err {err:.3e}"
        got[tile] = (out.get(), part.get())
    for tile in (native.TILE_PP256, native.TILE_AUTO):
        assert torch.equal(got[tile][0], got[native.TILE_64x64][0]) and torch.equal(got[tile][1], got[native.TILE_64x64][1]), \
            f"K split {ksplit}: tile {tile} differs in bits from the 64x64 tile"


@pytest.mark.parametrize("case", ["dense2", "dense4", "conv2", "conv3"])
def test_all_partial_k_split_and_its_finishing_kernel(lib, dt, case):
    from muggled_dpt_amd import native
    ksplit = int(case[-1])
    g = rng(ksplit + len(case))
    if case.startswith("dense"):
        M, N, K = 130, 256, 1024
        a = op(g.standard_normal((M, K)), dt)
        w = op(g.standard_normal((N, K)) / math.sqrt(K), dt)
        rows = f64(a)
        form = dict(a_hi=a, lda=K, amode=native.A_DENSE)
    else:  # 3x3 conv, Cin = 128 on 5 x 7: 18 K tiles, three ranges start in the middle of a 64-channel block's taps
        B, H, W, cin, N = 2, 5, 7, 128, 64
        M, K = B * H * W, 9 * cin
        a = op(g.standard_normal((B, H, W, cin)), dt)
        w = op(rs.pack_conv3(g.standard_normal((N, cin, 3, 3)) / math.sqrt(K)), dt)
        rows = rs.conv3_rows(f64(a), 1)
        form = dict(a_hi=a, lda=cin, amode=native.A_CONV3, Hi=H, Wi=W, Cin=cin, Ho=H, Wo=W, cstride=1)
    bias = g.standard_normal(N).astype(np.float32)
    planes_ref = rs.ksplit_planes(rows, f64(w), ksplit)
    ref = rs.generic(rs.product(rows, f64(w)), bias)
    bias_d = f32(bias)
    for tile in (native.TILE_AUTO, native.TILE_64x64, native.TILE_PP256):  # the all-partial form runs the 64x64 tile whatever is asked for
        o32, hi, lo, part = Out((M, N), torch.float32), Out((M, N), dt), Out((M, N), dt), Out((ksplit, M, N), torch.float32)
        form.update(w_hi=w, M=M, N=N, K=K, npass=1, ekind=native.E_GENERIC, tile=tile, bias=bias_d, out_f32=o32, out_hi=hi, out_lo=lo, relu_bf16=1, ldc=N,
                    ldr=N, ksplit=ksplit, ks_all=1, ks_part=part)
        what = f"ks_all {case} tile={tile}"
        assert launch(lib, **form) == 0, lib.mdpt_last_error()
        check_f32(part, np.stack(planes_ref), f"{what} planes")
        assert o32.untouched() and hi.untouched() and lo.untouched(), f"{what}: the GEMM wrote more than its partial planes"
        assert launch(lib, fn="mdpt_debug_ksplit_finish", **form) == 0, lib.mdpt_last_error()
        check_f32(o32, ref, f"{what} finished")
        check_split_of(hi, lo, o32.get(), dt, f"{what} finished", relu=True)


# ------------------------------------------------------------------------------------------------ npass 2 and 3, dense
@pytest.mark.parametrize("npass", [2, 3])
def test_split_operand_passes_on_dense_rows(lib, dt, npass):
    from muggled_dpt_amd import native
    M, N, K = 130, 128, 256
    g = rng(npass)
    a_hi, a_lo = split(g.standard_normal((M, K)), dt)
    w_hi, w_lo = split(g.standard_normal((N, K)) / math.sqrt(K), dt)
    ref = rs.pass_terms(f64(a_hi), f64(a_lo), f64(w_hi), f64(w_lo), npass)
    first = None
    for tile in TILES:
        out = Out((M, N), torch.float32)
        rc = launch(lib, a_hi=a_hi, a_lo=a_lo, w_hi=w_hi, w_lo=w_lo if npass == 3 else None, M=M, N=N, K=K, lda=K, npass=npass, amode=native.A_DENSE,
                    ekind=native.E_GENERIC, tile=tile, out_f32=out, ldc=N, ldr=N)
        assert rc == 0, lib.mdpt_last_error()
        check_f32(out, ref, f"npass={npass} tile={tile}")
        first = out.get() if first is None else first
        assert torch.equal(out.get(), first), f"npass={npass}: tile {tile} differs from tile {TILES[0]} in bits"


# ------------------------------------------------------------------------------------------------ wscale with acc_init (fp16 build)
def test_weight_scale_with_residual_initialised_accumulators_is_an_exact_rescaling(lib, request):
    """fp16 build only (the bf16 build ignores wscale): weights times s = 2^4 with wscale = {s, 1 / s} give the bits of the unscaled run."""
    from muggled_dpt_amd import native
    request.addfinalizer(lambda: native.check(lib, lib.mdpt_debug_set_operand_format(0)))
    native.check(lib, lib.mdpt_debug_set_operand_format(1))
    M, N, K, s = 130, 256, 256, 16.0
    g = rng(31)
    a, w1 = op(g.standard_normal((M, K)), torch.float16), op(g.standard_normal((N, K)) / math.sqrt(K), torch.float16)
    ws = (w1.float() * s).to(torch.float16)
    assert torch.equal(ws.float() / s, w1.float())  # the scaling is exact
    bias, resid = g.standard_normal(N).astype(np.float32), g.standard_normal((M, N)).astype(np.float32)
    ref = rs.generic(rs.product(f64(a), f64(w1)), bias, resid=resid)
    bias_d, scale_d = f32(bias), f32(np.array([s, 1.0 / s]))
    for tile in TILES:
        outs = []
        for w, wscale in ((w1, None), (ws, scale_d)):
            out = Out((M, N), torch.float32)
            out.buf[out.g:out.g + out.n] = f32(resid).reshape(-1)
            rc = launch(lib, a_hi=a, w_hi=w, M=M, N=N, K=K, lda=K, npass=1, amode=native.A_DENSE, ekind=native.E_GENERIC, tile=tile, bias=bias_d, resid=out,
                        out_f32=out, ldc=N, ldr=N, acc_init=1, wscale=wscale)
            assert rc == 0, lib.mdpt_last_error()
            check_f32(out, ref, f"acc_init wscale={'s' if wscale is not None else 'none'} tile={tile}")
            outs.append(out.get())
        assert torch.equal(outs[0], outs[1]), f"tile {tile}: the scaled run differs in bits from the unscaled one"


# ------------------------------------------------------------------------------------------------ refused combinations
def test_refused_combinations_launch_nothing(lib, dt):
    from muggled_dpt_amd import native
    M, N, K = 130, 256, 1024
    a, w = op(np.ones((M, K)), dt), op(np.ones((N, K)), dt)
    bias = f32(np.ones(1024))
    o32, hi, part, dep = Out((M, N), torch.float32), Out((M, N), dt), Out((4, M, N), torch.float32), Out((M,), torch.float32)
    base = dict(a_hi=a, w_hi=w, M=M, N=N, K=K, lda=K, npass=1, amode=native.A_DENSE, ekind=native.E_GENERIC, tile=0, bias=bias, out_f32=o32, ldc=N, ldr=N)
    qkv = dict(ekind=native.E_QKV, N=192, F=64, heads=1, qscale=0.125, q_hi=hi, k_hi=hi, vt_hi=hi, out_f32=None)
    refused = [
        dict(K=1000),                                                  # K % 64
        dict(N=252),                                                   # N % 8
        dict(npass=2),                                                 # activation split without a lo plane
        dict(npass=3, a_lo=a),                                         # three passes without a lo plane of the weights
        dict(ksplit=3, ks_part=part),                                  # 16 K tiles in three ranges
        dict(ksplit=2),                                                # no partial planes
        dict(ksplit=2, ks_part=part, out_hi=hi),                       # the split is for fp32 outputs
        dict(ksplit=2, ks_part=part, act=1),
        dict(ksplit=2, ks_part=part, ldw=2 * K),                       # no K range of wider rows under a split
        dict(ksplit=2, ks_part=part, amode=native.A_TOKENS, tok_np=13, tok_stride=16),
        dict(ksplit=2, ks_all=1, ks_part=part, acc_init=1, resid=o32),
        dict(ksplit=2, ks_all=1, ks_part=part, ekind=native.E_D2S, d2s_k=2, d2s_cout=64, Ho=10, Wo=13, out_hi=hi),
        dict(qkv, npad=13, npadv=16, M=26),                            # npad % 8
        dict(qkv, npad=16, npadv=20, M=32),                            # npadv % 8
        dict(qkv, npad=16, npadv=16, M=32, amode=native.A_TOKENS, tok_np=16, tok_stride=17),
        dict(ekind=native.E_PATCH, amode=native.A_TOKENS, tok_np=13, tok_stride=16, npad=16),
        dict(ekind=native.E_D2S, d2s_k=2, d2s_cout=60, N=240, Ho=10, Wo=13, out_hi=hi),  # cout % 8
        dict(ekind=native.E_HEAD, N=64, head_w=bias, head_b=bias, head_out=dep),        # the head is 32 wide
        dict(ekind=native.E_HEAD, N=32, head_w=bias, head_b=bias, head_out=dep),        # ... and a 3x3 conv
        dict(ekind=7),
    ]
    for over in refused:
        form = dict(base)
        form.update(over)
        assert launch(lib, **form) == INVALID, f"accepted: {over}"
        assert b"hip error" in lib.mdpt_last_error()
        assert o32.untouched() and hi.untouched() and part.untouched() and dep.untouched(), f"a refused launch wrote: {over}"
