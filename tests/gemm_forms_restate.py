"""Plain numpy float64 restatements of every operand and epilogue form of the GEMM family (csrc/mdpt_kernels.h GemmParams), one function
per form, written from the layouts its comments give - not from the epilogue code. Each takes the operands the kernel gets (already rounded
to the 16-bit operand format, so every product and sum is exact enough in float64 to serve as the truth) and returns every output buffer in
the kernel's layout. An element a form does NOT own (the cls and pad rows of the patch output, the columns [npad, npadv) of Vt) is NaN in the
returned array: the GPU tests require those bytes to come back untouched.

tests/test_gemm_forms_cpu.py proves each function against an independent torch formulation (F.conv2d, F.conv_transpose2d, a linear layer
followed by reshape / permute ...); tests/test_gpu_gemm_forms.py compares the kernels with them."""
import numpy as np

F64 = np.float64


def _f64(x):
    return None if x is None else np.asarray(x, dtype=F64)


# ---- weight layouts (the MDPT_PACK_* kinds of csrc/mdpt_kernels.h)
def pack_conv3(w):
    """MDPT_PACK_CONV3: [Cout][Cin][3][3] -> [Cout][9 Cin], k = (cb * 9 + ky * 3 + kx) * 64 + c with ci = cb * 64 + c."""
    w = _f64(w)
    cout, cin = w.shape[:2]
    out = np.zeros((cout, 9 * cin), F64)
    for cb in range(cin // 64):
        for ky in range(3):
            for kx in range(3):
                k0 = (cb * 9 + ky * 3 + kx) * 64
                out[:, k0:k0 + 64] = w[:, cb * 64:cb * 64 + 64, ky, kx]
    return out


def pack_convt(w):
    """MDPT_PACK_CONVT: [Cin][Cout][k][k] -> rows n = (ky * k + kx) * Cout + co, columns ci."""
    w = _f64(w)
    cin, cout, k, _ = w.shape
    out = np.zeros((k * k * cout, cin), F64)
    for ky in range(k):
        for kx in range(k):
            out[(ky * k + kx) * cout:(ky * k + kx + 1) * cout] = w[:, :, ky, kx].T
    return out


# ---- operand forms: the logical A [M, K] a launch multiplies
def token_rows(src, B, tok_np, tok_stride):
    """MDPT_A_TOKENS: logical row m = (b, p) reads source row b * tok_stride + 1 + p (the cls row and the pad rows are skipped)."""
    src = _f64(src)
    rows = [b * tok_stride + 1 + p for b in range(B) for p in range(tok_np)]
    return src[rows]


def conv3_rows(x, stride):
    """MDPT_A_CONV3: NHWC [B, Hi, Wi, Cin], 3x3, pad 1, stride `stride` -> the rows [B Ho Wo, 9 Cin] in the MDPT_PACK_CONV3 K order
    (Ho = ceil(Hi / stride)); taps outside the map are zero."""
    x = _f64(x)
    B, Hi, Wi, Cin = x.shape
    Ho, Wo = -(-Hi // stride), -(-Wi // stride)
    rows = np.zeros((B, Ho, Wo, 9 * Cin), F64)
    for y in range(Ho):
        for xo in range(Wo):
            for ky in range(3):
                for kx in range(3):
                    iy, ix = y * stride - 1 + ky, xo * stride - 1 + kx
                    if 0 <= iy < Hi and 0 <= ix < Wi:
                        for cb in range(Cin // 64):
                            k0 = (cb * 9 + ky * 3 + kx) * 64
                            rows[:, y, xo, k0:k0 + 64] = x[:, iy, ix, cb * 64:cb * 64 + 64]
    return rows.reshape(B * Ho * Wo, 9 * Cin)


def product(a, w, k0=0, k1=None):
    """A [M, K] W[N, K]^T over the K range [k0, k1)."""
    a, w = _f64(a), _f64(w)
    return a[:, k0:k1] @ w[:, k0:k1].T


def pass_terms(a_hi, a_lo, w_hi, w_lo, npass):
    """GemmParams::npass: 1 = A_hi W_hi; 2 = A_lo W_hi + A_hi W_hi; 3 = A_lo W_hi + A_hi W_lo + A_hi W_hi."""
    acc = product(a_hi, w_hi)
    if npass >= 2:
        acc = acc + product(a_lo, w_hi)
    if npass == 3:
        acc = acc + product(a_hi, w_lo)
    return acc


def ksplit_planes(a, w, ksplit):
    """GemmParams::ksplit: the bare partial sums of the ksplit equal K ranges, range z = plane z."""
    K = np.asarray(a).shape[1]
    ks = K // ksplit
    return [product(a, w, z * ks, (z + 1) * ks) for z in range(ksplit)]


# ---- epilogue forms
def _row_bias(bias, M, N, img_rows):
    """bias [N] shared, or a table [images, N]: row m uses row m // img_rows of it."""
    if bias is None:
        return np.zeros((M, N), F64)
    bias = _f64(bias)
    if bias.ndim == 1:
        return np.broadcast_to(bias, (M, N))
    return bias[np.arange(M) // img_rows]


def generic(acc, bias=None, bias_img_rows=0, act="none", gamma=None, resid=None):
    """MDPT_E_GENERIC: v = acc (+ bias[n]) -> act -> (* gamma[n]) (+ resid[m, n]); [M, N]."""
    acc = _f64(acc)
    M, N = acc.shape
    v = acc + _row_bias(bias, M, N, bias_img_rows)
    if act == "relu":
        v = np.maximum(v, 0.0)
    if gamma is not None:
        v = v * _f64(gamma)
    if resid is not None:
        v = v + _f64(resid)
    return v


def qkv(acc, bias, B, npad, npadv, heads, qscale, bias_img_rows=0):
    """MDPT_E_QKV: acc [B npad, 3F] (columns Q | K | V, head h = columns h * 64 .. + 63 of each) + bias -> Q * qscale and K head-major
    [B, heads, npad, 64], V transposed [B, heads, 64, npadv] whose columns [npad, npadv) are not written (NaN here)."""
    acc = _f64(acc)
    M, N = acc.shape
    Fd = heads * 64
    assert M == B * npad and N == 3 * Fd
    v = (acc + _row_bias(bias, M, N, bias_img_rows)).reshape(B, npad, 3, heads, 64)
    q = np.ascontiguousarray(v[:, :, 0].transpose(0, 2, 1, 3)) * qscale
    k = np.ascontiguousarray(v[:, :, 1].transpose(0, 2, 1, 3))
    vt = np.full((B, heads, 64, npadv), np.nan, F64)
    vt[..., :npad] = v[:, :, 2].transpose(0, 2, 3, 1)
    return q, k, vt


def patch(acc, bias, pos, B, tok_np, npad):
    """MDPT_E_PATCH: out[b * npad + 1 + p, n] = acc[b * tok_np + p, n] + bias[n] (+ pos[p, n]); the cls row 0 and the rows from 1 + tok_np on of every
    image are not written (NaN here)."""
    acc = _f64(acc)
    N = acc.shape[1]
    v = acc.reshape(B, tok_np, N) + _f64(bias)
    if pos is not None:
        v = v + _f64(pos)[None]
    out = np.full((B, npad, N), np.nan, F64)
    out[:, 1:1 + tok_np] = v
    return out.reshape(B * npad, N)


def d2s(acc, bias, B, Ho, Wo, k, cout):
    """MDPT_E_D2S: a transposed conv with kernel == stride == k as a GEMM, n = (ky * k + kx) * cout + co -> NHWC [B, Ho k, Wo k, cout] (+ bias[co])."""
    acc = _f64(acc).reshape(B, Ho, Wo, k, k, cout)
    out = acc.transpose(0, 1, 3, 2, 4, 5).reshape(B, Ho * k, Wo * k, cout)
    return out + _f64(bias)


def head(acc, bias, head_w, head_b, sigmoid):
    """MDPT_E_HEAD (N = 32): depth[m] = final(sum_n relu(acc[m, n] + bias[n]) * head_w[n] + head_b), final = ReLU or the logistic sigmoid."""
    s = np.maximum(_f64(acc) + _f64(bias), 0.0) @ _f64(head_w) + float(head_b)
    return 1.0 / (1.0 + np.exp(-s)) if sigmoid else np.maximum(s, 0.0)
