"""The HBM-bound helper kernels of csrc/elementwise.hip (the ew_*.inc files) called directly through their extern "C" launchers, in both operand
builds (..._bf16 / ..._f16), on torch's current stream with torch tensors as buffers. Inputs are seeded uniform in [-4, 4]: no fp16 / fp8
conversion saturates. What is bit-exact is asserted bit for bit (the kernels run with fp contraction off where that matters, and HIP's fp32
division is correctly rounded); only LayerNorm against fp64 has a tolerance."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FORMATS = {"bf16": torch.bfloat16, "f16": torch.float16}
INVALID = 1  # hipErrorInvalidValue
_P, _I, _Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
ARGS = {
    "layernorm": [_P, _P, _P, _P, _P, _P, _I, _I, _P, _Z, _I],
    "layernorm_addp": [_P, _P, _Z, _I, _P, _P, _P, _P, _P, _I, _I, _P, _Z, _I],
    "zero_vt_pad": [_P, _P, _I, _I, _I, _P],
    "upsample": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _Z, _I],
    "upsample_bf16": [_P, _P, _I, _I, _I, _I, _I, _I, _P],
    "tokens_import": [_P, _P, _P, _I, _I, _I, _I, _P, _Z, _I],
    "tokens_export": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _Z],
    "nchw_to_nhwc": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _Z, _I],
    "nhwc_to_nchw": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P],
}


def launch(name, fmt, *args):
    """mdpt_launch_<name>_<fmt>(*args, stream inserted where the signature has it) on torch's current stream -> hipError_t; tensors pass as pointers"""
    from muggled_dpt_amd import native
    fn = getattr(native.load(), f"mdpt_launch_{name}_{fmt}")
    fn.restype, fn.argtypes = ctypes.c_int, ARGS[name]
    vals = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    vals = [torch.cuda.current_stream().cuda_stream if a == "stream" else a for a in vals]
    rc = fn(*vals)
    torch.cuda.synchronize()
    return rc


def uniform(seed, *shape):
    x = (torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * 8 - 4).float()
    assert float(x.abs().max()) <= 4.0  # no fp16 / fp8 conversion of these values saturates
    return x


UNWRITTEN = -7.0  # what output buffers hold before a launch: exact in every format, outside the inputs' range, and - unlike NaN - harmless to
# whichever later test is handed the freed memory as an uninitialised buffer


def unwritten(*shape, dtype=torch.float32):
    return torch.full(shape, UNWRITTEN, device="cuda", dtype=dtype)


def bits(t):
    return t.cpu().view(torch.int16) if t.dtype in (torch.bfloat16, torch.float16) else t.cpu()


def planes_of(v, dtype):
    """the (hi, lo) operand planes of fp32 values: hi = v.to(dtype), lo = (v - hi).to(dtype)"""
    hi = v.to(dtype)
    return hi, (v - hi.float()).to(dtype)


def upsample_restate(src, Ho, Wo):
    """align_corners=True bilinear resize of NHWC float32 `src` in the kernels' own operation order, every operation rounded to float32 (numpy)"""
    f = np.float32
    B, Hi, Wi, C = src.shape
    sy = f(Hi - 1) / f(Ho - 1) if Ho > 1 else f(0)
    sx = f(Wi - 1) / f(Wo - 1) if Wo > 1 else f(0)
    fy, fx = sy * np.arange(Ho, dtype=f), sx * np.arange(Wo, dtype=f)
    y0, x0 = fy.astype(np.int32), fx.astype(np.int32)
    y1, x1 = y0 + (y0 < Hi - 1), x0 + (x0 < Wi - 1)
    ly, lx = (fy - y0.astype(f))[None, :, None, None], (fx - x0.astype(f))[None, None, :, None]
    v00, v01 = src[:, y0][:, :, x0], src[:, y0][:, :, x1]
    v10, v11 = src[:, y1][:, :, x0], src[:, y1][:, :, x1]
    out = (f(1) - ly) * ((f(1) - lx) * v00 + lx * v01) + ly * ((f(1) - lx) * v10 + lx * v11)
    assert out.dtype == f
    return out


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("C", [12, 64])  # upsample_kernel<4> / <8>
def test_upsample_direct_is_the_float32_restatement(fmt, C):
    dtype = FORMATS[fmt]
    B, Hi, Wi, Ho, Wo = 2, 5, 7, 9, 16
    x = uniform(C, B, Hi, Wi, C)
    want = torch.from_numpy(upsample_restate(x.numpy(), Ho, Wo))
    xd = x.cuda()
    f32 = unwritten(B, Ho, Wo, C)
    assert launch("upsample", fmt, xd, None, None, f32, B, Hi, Wi, Ho, Wo, C, "stream", 0, 0) == 0
    assert torch.equal(f32.cpu(), want)
    hi, lo, f32 = unwritten(B, Ho, Wo, C, dtype=dtype), unwritten(B, Ho, Wo, C, dtype=dtype), unwritten(B, Ho, Wo, C)
    assert launch("upsample", fmt, xd, hi, lo, f32, B, Hi, Wi, Ho, Wo, C, "stream", 0, 0) == 0
    want_hi, want_lo = planes_of(want, dtype)
    assert torch.equal(f32.cpu(), want) and torch.equal(bits(hi), bits(want_hi)) and torch.equal(bits(lo), bits(want_lo))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", [(64, 131, 131, 261, 261), (128, 93, 93, 257, 257)])  # >= 65536 output pixels, 7 (Hi - 1) <= 5 (Ho - 1), partial tiles on both edges
def test_upsample_tiled_equals_direct(fmt, shape):
    dtype = FORMATS[fmt]
    C, Hi, Wi, Ho, Wo = shape
    assert Ho * Wo >= 65536 and 7 * (Hi - 1) <= 5 * (Ho - 1) and Ho % 8 and Wo % 8
    xd = uniform(Hi, 1, Hi, Wi, C).cuda()
    out = {}
    for path in ("tiled", "direct"):  # out_f32 == null: tiled; out_f32 set: direct
        hi, lo = unwritten(1, Ho, Wo, C, dtype=dtype), unwritten(1, Ho, Wo, C, dtype=dtype)
        f32 = unwritten(1, Ho, Wo, C) if path == "direct" else None
        assert launch("upsample", fmt, xd, hi, lo, f32, 1, Hi, Wi, Ho, Wo, C, "stream", 0, 0) == 0
        out[path] = (bits(hi), bits(lo))
        assert not (hi.float() == UNWRITTEN).any() and not (lo.float() == UNWRITTEN).any()  # every output element was written
    assert torch.equal(out["tiled"][0], out["direct"][0]) and torch.equal(out["tiled"][1], out["direct"][1])


@pytest.mark.parametrize("fmt", FORMATS)
def test_upsample_to_one_output_row(fmt):
    """Ho = 1: sy = 0, every output row reads source row 0 (and row 1 with weight 0)"""
    dtype = FORMATS[fmt]
    B, Hi, Wi, Ho, Wo, C = 1, 3, 4, 1, 9, 64
    x = uniform(3, B, Hi, Wi, C)
    want = torch.from_numpy(upsample_restate(x.numpy(), Ho, Wo))
    hi, lo = unwritten(B, Ho, Wo, C, dtype=dtype), unwritten(B, Ho, Wo, C, dtype=dtype)
    assert launch("upsample", fmt, x.cuda(), hi, lo, None, B, Hi, Wi, Ho, Wo, C, "stream", 0, 0) == 0
    want_hi, want_lo = planes_of(want, dtype)
    assert torch.equal(bits(hi), bits(want_hi)) and torch.equal(bits(lo), bits(want_lo))


@pytest.mark.parametrize("fmt", FORMATS)
def test_upsample_bf16src_is_the_float32_restatement_rounded(fmt):
    """operand-format map -> operand-format map (up_bf16.h): the same expression on the widened source, rounded once"""
    dtype = FORMATS[fmt]
    B, Hi, Wi, Ho, Wo, C = 2, 5, 7, 9, 16, 16
    src = uniform(16, B, Hi, Wi, C).to(dtype)
    want = torch.from_numpy(upsample_restate(src.float().numpy(), Ho, Wo)).to(dtype)
    out = unwritten(B, Ho, Wo, C, dtype=dtype)
    assert launch("upsample_bf16", fmt, src.cuda(), out, B, Hi, Wi, Ho, Wo, C, "stream") == 0
    assert torch.equal(bits(out), bits(want))


F8_LO_SHIFT = 11  # the residue bytes are e5m2((x - hi) 2^11) (csrc/f8_cross.h; 2^16 before the residue clamp fix, which saturated residues of |x| >= 2048)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("skip_cls", [0, 1])
def test_tokens_import_export_round_trip(fmt, skip_cls):
    dtype = FORMATS[fmt]
    B, N, npad, F = 2, 5, 8, 12
    x = uniform(5 + skip_cls, B, N, F)
    hi, lo = unwritten(B, npad, F, dtype=dtype), unwritten(B, npad, F, dtype=dtype)
    assert launch("tokens_import", fmt, x.cuda(), hi, lo, B, N, npad, F, "stream", 0, 0) == 0
    want_hi, want_lo = planes_of(x, dtype)
    assert torch.equal(bits(hi[:, :N]), bits(want_hi)) and torch.equal(bits(lo[:, :N]), bits(want_lo))
    assert not hi[:, N:].float().any() and not lo[:, N:].float().any()  # pad rows are zero
    out = unwritten(B, N - skip_cls, F)
    assert launch("tokens_export", fmt, hi, lo, None, out, B, N, npad, F, skip_cls, "stream", 0) == 0
    assert torch.equal(out.cpu(), (want_hi.float() + want_lo.float())[:, skip_cls:])
    if fmt != "f16":
        return
    # the fp8 form an F8 consumer reads: residue bytes e5m2((x - hi) 2^F8_LO_SHIFT), then the a8 plane e5m2(hi) out_f8 bytes behind them
    n, scale = B * npad * F, float(2 ** F8_LO_SHIFT)
    lo8 = torch.zeros(2 * n, device="cuda", dtype=torch.uint8)
    assert launch("tokens_import", fmt, x.cuda(), hi, lo8, B, N, npad, F, "stream", n, 1) == 0
    xp = torch.zeros(B, npad, F)
    xp[:, :N] = x
    hp = xp.to(dtype)
    want_r = ((xp - hp.float()) * scale).to(torch.float8_e5m2)
    assert torch.equal(lo8[:n].cpu(), want_r.view(torch.uint8).reshape(-1))
    assert torch.equal(lo8[n:].cpu(), hp.float().to(torch.float8_e5m2).view(torch.uint8).reshape(-1))
    assert launch("tokens_export", fmt, hi, lo8, None, out, B, N, npad, F, skip_cls, "stream", n) == 0
    assert torch.equal(out.cpu(), (hp.float() + want_r.float() * (1.0 / scale))[:, skip_cls:N])


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("relu", [0, 1])
def test_nchw_nhwc_round_trip(fmt, relu):
    dtype = FORMATS[fmt]
    B, C, Cp, H, W = 2, 3, 8, 5, 7
    x = uniform(7 + relu, B, C, H, W)
    f32, hi, lo = unwritten(B, H, W, Cp), unwritten(B, H, W, Cp, dtype=dtype), unwritten(B, H, W, Cp, dtype=dtype)
    assert launch("nchw_to_nhwc", fmt, x.cuda(), f32, hi, lo, relu, B, H, W, C, Cp, "stream", 0, 0) == 0
    nhwc = x.permute(0, 2, 3, 1)
    assert torch.equal(f32[..., :C].cpu(), nhwc)  # the fp32 output is not ReLU'd
    want_hi, want_lo = planes_of(nhwc.clamp(min=0) if relu else nhwc, dtype)
    assert torch.equal(bits(hi[..., :C]), bits(want_hi)) and torch.equal(bits(lo[..., :C]), bits(want_lo))
    assert not f32[..., C:].any() and not hi[..., C:].float().any() and not lo[..., C:].float().any()  # pad channels are zero
    out = unwritten(B, C, H, W)
    assert launch("nhwc_to_nchw", fmt, None, hi, lo, out, B, H, W, C, Cp, "stream") == 0
    assert torch.equal(out.cpu(), (want_hi.float() + want_lo.float()).permute(0, 3, 1, 2))
    if fmt != "f16":
        return
    # the fp8 form an F8 consumer reads, as in the token import: residue bytes, then the a8 plane out_f8 bytes behind them (ReLU'd like the planes)
    n, scale = B * H * W * Cp, float(2 ** F8_LO_SHIFT)
    lo8 = torch.zeros(2 * n, device="cuda", dtype=torch.uint8)
    assert launch("nchw_to_nhwc", fmt, x.cuda(), f32, hi, lo8, relu, B, H, W, C, Cp, "stream", n, 1) == 0
    vp = torch.zeros(B, H, W, Cp)
    vp[..., :C] = nhwc.clamp(min=0) if relu else nhwc
    hp = vp.to(dtype)
    assert torch.equal(bits(hi), bits(hp))
    assert torch.equal(lo8[:n].cpu(), ((vp - hp.float()) * scale).to(torch.float8_e5m2).view(torch.uint8).reshape(-1))
    assert torch.equal(lo8[n:].cpu(), hp.float().to(torch.float8_e5m2).view(torch.uint8).reshape(-1))


LN_F = [256, 260, 512, 516, 1028, 1540]  # NV = 1, 2, 2, 4, 6, 8: every case of the row-width dispatch, at its lower edge where it has one
LN_TOL = 4 * 9.472e-07  # 4 x the largest error measured on the commit before the split (docstring of the test below)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("F", LN_F)
def test_layernorm_dispatch_against_fp64_and_addp_bitwise(fmt, F):
    """rows = 5 (a partial workgroup of 4 rows). out_f32 against fp64 LayerNorm (eps 1e-6), and layernorm_addp with two partial sums against
    layernorm of the pre-summed rows, bit for bit, the sum written back to x.
    No other test bounds this kernel's own output, so the tolerance is measured: on the commit before the file was split the largest |out_f32 - fp64|
    at these shapes was 6.745e-07 (F = 256), 6.969e-07 (260), 8.007e-07 (512), 9.164e-07 (516), 9.472e-07 (1028), 8.825e-07 (1540), the same in
    both operand builds (outputs of magnitude up to ~12: a few fp32 ulps); the bound is 4 x the largest, 3.789e-06."""
    dtype = FORMATS[fmt]
    rows = 5
    x, gamma, beta = uniform(F, rows, F), uniform(F + 1, F), uniform(F + 2, F)
    xd64 = x.double()
    mean, var = xd64.mean(-1, keepdim=True), xd64.var(-1, unbiased=False, keepdim=True)
    ref = (xd64 - mean) / torch.sqrt(var + 1e-6) * gamma.double() + beta.double()
    hi, lo, f32 = unwritten(rows, F, dtype=dtype), unwritten(rows, F, dtype=dtype), unwritten(rows, F)
    assert launch("layernorm", fmt, x.cuda(), gamma.cuda(), beta.cuda(), hi, lo, f32, rows, F, "stream", 0, 0) == 0
    err = float((f32.cpu().double() - ref).abs().max())
    print(f"layernorm {fmt} F={F}: max abs err against fp64 {err:.3e}")
    assert err <= LN_TOL
    want_hi, want_lo = planes_of(f32.cpu(), dtype)
    assert torch.equal(bits(hi), bits(want_hi)) and torch.equal(bits(lo), bits(want_lo))
    parts = uniform(F + 3, 2, rows, F)
    xs = (x + parts[0]) + parts[1]
    base, xin = [unwritten(rows, F, dtype=dtype), unwritten(rows, F, dtype=dtype), unwritten(rows, F)], xs.cuda()
    assert launch("layernorm", fmt, xin, gamma.cuda(), beta.cuda(), *base, rows, F, "stream", 0, 0) == 0
    got, xio = [unwritten(rows, F, dtype=dtype), unwritten(rows, F, dtype=dtype), unwritten(rows, F)], x.cuda()
    assert launch("layernorm_addp", fmt, xio, parts.cuda(), rows * F, 2, gamma.cuda(), beta.cuda(), *got, rows, F, "stream", 0, 0) == 0
    assert torch.equal(xio.cpu(), xs)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(got, base))


@pytest.mark.parametrize("fmt", FORMATS)
def test_rejected_arguments_launch_nothing(fmt):
    dtype = FORMATS[fmt]
    x, g, out = uniform(1, 5, 8).cuda(), uniform(2, 8).cuda(), unwritten(5, 8)
    hi = unwritten(5, 8, dtype=dtype)
    assert launch("layernorm", fmt, x, g, g, hi, None, out, 5, 6, "stream", 0, 0) == INVALID                  # F & 3
    assert launch("layernorm_addp", fmt, x, x, 40, 1, g, g, hi, None, out, 5, 6, "stream", 0, 0) == INVALID   # F & 3
    assert launch("upsample", fmt, x, hi, None, out, 1, 1, 1, 1, 1, 6, "stream", 0, 0) == INVALID             # C & 3
    assert launch("upsample_bf16", fmt, hi, hi, 1, 1, 1, 1, 1, 12, "stream") == INVALID                       # C & 7
    assert launch("zero_vt_pad", fmt, hi, None, 5, 8, 8, "stream") == 0                                       # npadv == N: nothing to do
    assert (out == UNWRITTEN).all() and (hi.float() == UNWRITTEN).all()
