"""Every form of the fused attention (csrc/attention.hip, 14 attn_kernel instantiations in each operand build) and the diagnostic weights dump on
their own operands (test hooks mdpt_debug_attention_form / mdpt_debug_attn_weights_form), against the float64 restatements of
tests/attention_restate.py (proven on the CPU by tests/test_attention_forms_cpu.py, which also shows that the case table reaches all 14
instantiations and that the window operands keep the score contract of the fixed-reference form). `pytest -m gpu`.

Operands are exact 16-bit planes (hi, and lo for the three-pass form); the float64 reference is computed on hi (+ lo). Q / K rows [N, npad) hold
+-1e4 (a leaked pad key would dominate the softmax), Vt columns [N, npadv) are zero as the kernel requires, bias tables hold a distinct random
value per entry and head. Every output buffer is filled with a sentinel and has guard rows in front and behind: guards, the pad columns
[F, out_ld) and lo planes that were not passed must come back bit-identical; in window mode every image row must have been written.

Bounds, per element, with A = sum_k P |v| in float64 on the same operands and u = 2^-9 (bf16) / 2^-12 (fp16):
  single pass (and the latency form)  |got - ref| <= (4 u + 2^-16) A (+ the fp16 term below): one rounding of P (the denominator sums the unrounded
                                      values), one rounding of the output, a slack for the fp32 accumulation and v_exp_f32.
                                      u is half a spacing relative to the TOP of a binade: round-to-nearest to p = 8 / 11 significant bits
                                      leaves half a spacing 2^(e - p) on a value in [2^e, 2^(e + 1)), which is 2^-p = 2 u of a value at the
                                      bottom of the binade, so each of the two roundings costs up to 2 u. (Measured: bf16 up to 7.69e-3 A, fp16
                                      up to 9.32e-4 A.)
  fp16 only                           + 2^-25 (1 + (sum_k |v|) max_k P): fp16 values below 2^-14 are subnormal and round with an absolute error of up
                                      to 2^-25 whatever their size. That holds for the output, and for every P: the kernel's reference point is
                                      a score the row attains, so its denominator is at least 1 / max_k P. (Measured without the term: window of
                                      144 tokens, synthetic regions, 1.85e-3 A on an output of 1e-5.) bf16 has fp32's exponent range: no such term.
                                      The lo plane of the three-pass form cannot go below that spacing either, so the values are drawn
                                      with |v| >= 0.25 in every case: a one-hot row then has no subnormal output, where three passes could not beat one.
  latency form against the unsplit launch: twice the single-pass bound;
  three pass (hi + lo)                not derivable here (the dropped lo * lo term moves the scores): measured, asserted at four times the
                                      measurement, and on every case below the single-pass error of the same case and format;
  weights dump                        |got - P| measured likewise; rows sum to 1 within N 2^-23.
MEASURED holds the measurements (MI355X, 2026-10-21; the largest value over the cases named beside each entry).

The rows at the deferred-maximum threshold (a key just under kDeferMax = 5.5 above a row's running reference point, one just over it, one of them
in the last partial tile) are built into the operands from the float64 scores and checked there after rounding (test_threshold_rows_...): for
head dim 64 by scaling two keys, for the windows (the fp16 build tracks a maximum there, in log2 units) inside the score contract through two
table entries of a query with two copies of its own key (attention_restate.swin_threshold_rows: every multi-tile window, the heads with a logit
scale of 16 or more - the contract leaves no room below that; the 12 x 12 windows have the partial last tile, in the narrow, wide and three-pass
forms and their twins without 4-key runs)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import attention_restate as rs

pytestmark = pytest.mark.gpu

SENT = 7.0
INVALID = 1  # hipErrorInvalidValue
DEFER, defer_walk = rs.DEFER, rs.defer_walk
# largest |got - ref| / A of the three-pass form and largest |got - P| of the weights dump per operand format
MEASURED = {
    # bf16: win_8x8_x3 without regions (head dim 64: at most 3.19e-5, beit_x3); fp16: win_7x7_x3 with the shifted-window regions (head dim 64: at
    # most 2.14e-6, beit_x3)
    "x3": {"bf16": 3.5912e-04, "fp16": 1.4821e-05},
    # bf16: win_7x7_x3 without regions; fp16: win_7x7 with the shifted-window regions (head dim 64: at most 7.82e-7)
    "weights": {"bf16": 8.9739e-06, "fp16": 8.5909e-06},
}


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


def fmt(dt):
    return "fp16" if dt == torch.float16 else "bf16"


def unit(dt):
    return 2.0 ** -12 if dt == torch.float16 else 2.0 ** -9


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


def launch(lib, fn="mdpt_debug_attention_form", extra=(), **kw):
    from muggled_dpt_amd import native
    f = native.MdptAttnForm()
    for k, v in kw.items():
        if v is None:
            continue
        setattr(f, k, v.ptr if isinstance(v, Out) else (v.data_ptr() if torch.is_tensor(v) else v))
    rc = getattr(lib, fn)(ctypes.byref(f), *[e.ptr for e in extra], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


INT_FIELDS = ("B", "heads", "N", "npad", "npadv", "F", "x3", "bias_elen", "head_dim", "win_nw", "region_ld", "bias_run4", "bias_row", "bias_ww", "out_ld",
              "allow_split_kv")


def ints(case):
    return {k: int(case[k]) for k in INT_FIELDS if case.get(k)}


def t32(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))


def f64(t):
    return t.detach().cpu().double().numpy()


class Ops:
    """device planes of one launch and the float64 values they hold"""

    def __init__(self, q, k, v, case, dt, seed, lo=None):
        """q, k, v [B, heads, N, hd] float64 -> Q / K [B, heads, npad, hd] with +-1e4 pad rows, Vt [B, heads, hd, npadv] with zero pad columns;
        lo planes whenever the case is three-pass (or lo is forced)"""
        B, H, N, hd = q.shape
        npad, npadv = case["npad"], case["npadv"]
        g = torch.Generator().manual_seed(seed)
        lo = bool(case["x3"]) if lo is None else lo
        self.N, self.dev = N, {}
        for name, x in (("q", q), ("k", k)):
            full = (torch.randint(0, 2, (B, H, npad, hd), generator=g).float() * 2 - 1) * 1.0e4
            full[:, :, :N] = t32(x)
            hi = full.to(dt)
            self.dev[name + "_hi"] = hi.cuda()
            val = hi[:, :, :N].double()
            if lo:
                l = (full - hi.float()).to(dt)
                l[:, :, N:] = hi[:, :, N:]  # garbage in the lo plane's pad rows too
                self.dev[name + "_lo"] = l.cuda()
                val = val + l[:, :, :N].double()
            setattr(self, name, val.numpy())
        vt = torch.zeros(B, H, hd, npadv)
        vt[..., :N] = t32(v).transpose(2, 3)
        hi = vt.to(dt)
        self.dev["vt_hi"] = hi.cuda()
        val = hi[..., :N].double()
        if lo:
            l = (vt - hi.float()).to(dt)
            self.dev["vt_lo"] = l.cuda()
            val = val + l[..., :N].double()
        self.v = val.transpose(2, 3).numpy()

    def hi_only(self, case):
        """the same hi planes as a single-pass launch: (device planes, q, k, v float64)"""
        o = Ops.__new__(Ops)
        o.N = self.N
        o.dev = {n: t for n, t in self.dev.items() if n.endswith("_hi")}
        o.q, o.k = (f64(self.dev[n + "_hi"][:, :, :self.N]) for n in ("q", "k"))
        o.v = f64(self.dev["vt_hi"][..., :self.N]).transpose(0, 1, 3, 2)
        return o

    def take(self, nb):
        """the first nb batch entries (views of the same device planes)"""
        o = Ops.__new__(Ops)
        o.N, o.dev = self.N, {n: t[:nb].contiguous() for n, t in self.dev.items()}
        o.q, o.k, o.v = self.q[:nb], self.k[:nb], self.v[:nb]
        return o


def run(lib, dt, case, ops, tables=None, x3=None, rows=None, rowmap=None, what="", **over):
    """one launch into sentinel-filled buffers -> output [B, heads, N, hd] float64 in batch (window) order (hi + lo for three-pass) and the raw hi
    plane; everything the launch does not own is checked here"""
    c = dict(case, **over)
    x3 = bool(c["x3"]) if x3 is None else x3
    c["x3"] = int(x3)
    B, H, N, hd, F = c["B"], c["heads"], c["N"], c.get("head_dim") or 64, c["F"]
    ld = c.get("out_ld") or F
    rows = rows if rows is not None else (B * N if c.get("rowmap") else B * c["npad"])
    o_hi, o_lo = Out((rows, ld), dt), Out((rows, ld), dt)
    planes = {n: t for n, t in ops.dev.items() if x3 or n.endswith("_hi")}
    kw = dict(ints(c), **planes, **(tables or {}), out_hi=o_hi, out_lo=o_lo if x3 else None)
    rc = launch(lib, **kw)
    assert rc == 0, f"{what}: {lib.mdpt_last_error()}"
    hi, lo = o_hi.get(), o_lo.get()
    assert o_hi.guards_ok() and o_lo.guards_ok(), f"{what}: wrote into the guard rows"
    assert bool((hi[:, F:] == SENT).all()) and bool((lo[:, F:] == SENT).all()), f"{what}: wrote into the pad columns [F, out_ld)"
    if not x3:
        assert o_lo.untouched(), f"{what}: the lo plane was not passed"
    got = hi[:, :F].double() + (lo[:, :F].double() if x3 else 0.0)
    if c.get("rowmap"):
        written = (hi[:, :F].reshape(rows, H, hd) != SENT).any(-1)
        assert bool(written.all()), f"{what}: {int((~written).sum())} (image row, head) blocks were never written"
        nw = c["win_nw"]
        idx = (torch.arange(B)[:, None] // nw * nw * N + torch.from_numpy(rowmap).long().view(nw, N).repeat(B // nw, 1)).flatten()
        got, hi = got[idx].view(B, N, H, hd), hi[idx][:, :F].reshape(B, N, H, hd)
    else:
        got, hi = got.view(B, c["npad"], H, hd)[:, :N], hi[:, :F].reshape(B, c["npad"], H, hd)[:, :N]
    return got.permute(0, 2, 1, 3).numpy(), hi.permute(0, 2, 1, 3).contiguous()


def ratio(got, ref, A):
    return float((np.abs(got - ref) / A).max())


def check_single(got, ref, A, dt, what, P, v, mul=1.0):
    """P, v: the float64 probabilities and values of the same operands (the fp16 subnormal term of the module docstring)"""
    tol = (4 * unit(dt) + 2.0 ** -16) * A
    if dt == torch.float16:
        tol = tol + 2.0 ** -25 * (1.0 + np.abs(v).sum(-2, keepdims=True) * P.max(-1, keepdims=True))
    tol = mul * tol
    err = np.abs(got - ref)
    print(f"MEASURE single {fmt(dt)} {what}: max |got - ref| / A = {ratio(got, ref, A):.4e}, max |got - ref| / bound = {float((err / tol).max()):.4f}")
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    i = np.unravel_index(np.argmax(err - tol), err.shape)
    assert (err <= tol).all(), f"{what}: |got - ref| = {err[i]:.4e} > {tol[i]:.4e} at {i} (ratio {err[i] / A[i]:.4e})"


def check_x3(got, ref, A, single_ratio, dt, what):
    r = ratio(got, ref, A)
    print(f"MEASURE x3 {fmt(dt)} {what}: max |got - ref| / A = {r:.4e} (single pass on the hi planes: {single_ratio:.4e})")
    m = MEASURED["x3"][fmt(dt)]
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    assert r <= 4 * m, f"{what}: three-pass error {r:.4e} above four times the recorded {m}"
    assert r < single_ratio, f"{what}: three-pass error {r:.4e} is not below the single-pass error {single_ratio:.4e}: the lo planes do nothing"


# ------------------------------------------------------------------------------------------------ operands, head dim 64
_PLAIN = {}


def plain_ops(name, dt):
    """operands, tables and the float64 reference of a head-dim-64 case: built once per (case, format), shared by every test that runs it"""
    key = (name, dt)
    if key in _PLAIN:
        return _PLAIN[key]
    c = rs.CASES[name]
    B, H, N = c["B"], c["heads"], c["N"]
    seed = {"wide_twin": "wide", "beit_wide_twin": "beit_wide"}.get(name, name)
    g = np.random.default_rng(sum(map(ord, seed)))
    q = g.standard_normal((B, H, N, 64)) * 0.25
    k = g.standard_normal((B, H, N, 64))
    v = g.standard_normal((B, H, N, 64))
    v = np.sign(v) * (0.25 + np.abs(v))  # (module docstring: no fp16-subnormal outputs on one-hot rows)
    tables, bias = None, None
    if c["kind"] == "beit":
        tq, tk, elen = rs.beit_tables(*c["grid"], c["npad"])
        lut = (g.standard_normal((H, elen)) * math.sqrt(2.0)).astype(np.float32)
        tables = dict(bias_lut=torch.from_numpy(lut).cuda(), tq=torch.from_numpy(tq).cuda(), tk=torch.from_numpy(tk).cuda())
        bias = lut.astype(np.float64)[:, tq[:N, None] - tk[None, :N]][None]
    # the threshold rows: key ka (in the last, partial tile when there is one) scores just under the reference point + DEFER for query qa, key kb
    # just over it for query qb, key kc far over it for query qc; placed from the float64 scores of the rounded operands of (batch 0, each head)
    rnd = lambda x: t32(x).to(dt).double().numpy()
    qr = rnd(q)
    last = (N - 1) // 64 * 64
    picks = ((3, N - 1, -0.25), (N // 2, max(last - 2, 1) if N > 64 else N - 3, +0.25), (N - 2, N - 2 if N - 2 >= last else N - 1, 40.0))
    picks = [p for i, p in enumerate(picks) if all(p[1] != o[1] for o in picks[:i])]
    for qi, ki, d in sorted(picks, key=lambda p: -abs(p[2])):  # the far key first: it moves other rows' scores the most
        for b in range(min(B, 2)):
            for h in range(H):
                s_row = qr[b, h, qi] @ rnd(k[b, h]).T + (bias[0, h, qi] if bias is not None else 0.0)
                m = defer_walk(np.delete(s_row, ki) if ki >= last else s_row, ki if ki < last else N - 1)
                want = m + DEFER + d - (bias[0, h, qi, ki] if bias is not None else 0.0)
                k[b, h, ki] = qr[b, h, qi] * want / (qr[b, h, qi] @ qr[b, h, qi])
    ops = Ops(q, k, v, c, dt, seed=N)
    ref = rs.attention(ops.q, ops.k, ops.v, bias)
    _PLAIN[key] = (c, ops, tables, bias, ref, picks)
    return _PLAIN[key]


def single_case(lib, dt, name, **over):
    c, ops, tables, bias, (ref, P, A), picks = plain_ops(name, dt)
    got, hi = run(lib, dt, c, ops, tables, what=name, **over)
    return c, ops, tables, bias, ref, A, got, hi, P


def test_threshold_rows_sit_where_they_should(dt):
    """(no launch) after rounding, the constructed keys are within 0.5 of the threshold on the intended side, in every head of image 0"""
    for name in ("narrow_linear", "tile_65", "beit_12x9", "split_325"):
        c, ops, tables, bias, _, picks = plain_ops(name, dt)
        N, last = c["N"], (c["N"] - 1) // 64 * 64
        for qi, ki, d in picks[:2]:
            for h in range(c["heads"]):
                s_row = ops.q[0, h, qi] @ ops.k[0, h].T + (bias[0, h, qi] if bias is not None else 0.0)
                m = defer_walk(np.delete(s_row, ki) if ki >= last else s_row, ki if ki < last else N - 1)
                gap = s_row[ki] - (m + DEFER)
                assert (0 < gap < 0.5) if d > 0 else (-0.5 < gap < 0), f"{name} head {h} query {qi} key {ki}: {gap:+.3f} from the threshold"


def test_window_threshold_rows_sit_where_they_should(dt):
    """(no launch) on the values the planes hold, ka is within 0.5 (log2 units) under the threshold and kb within 0.5 over it, in window 0 of
    every head with room, for the narrow, wide and three-pass forms"""
    for name in ("win_12x12", "win_12x12_wide", "win_12x12_x3", "win_16x20_wide", "win_24x24"):
        c, ops, dev, bias, regions, extra = swin_ops(name, dt)
        assert len(extra["pairs"]) >= (2 if c["heads"] == 4 else 1), name
        for (h, qi, ka, kb), (under, over) in zip(extra["pairs"], rs.swin_threshold_gaps(c, ops.q, ops.k, extra["lut"], extra["pairs"])):
            assert -0.5 < under < 0 < over < 0.5, f"{name} head {h} query {qi}: ka {under:+.3f}, kb {over:+.3f} from the threshold"
            assert "12x12" not in name or kb >= 128


# ------------------------------------------------------------------------------------------------ plain and BEiT, single pass
SINGLE = [n for n, c in {**rs.PLAIN_CASES, **rs.BEIT_CASES}.items() if not c["x3"] and not c["allow_split_kv"] and not n.endswith("_twin")]


@pytest.mark.parametrize("name", SINGLE)
def test_single_pass_against_float64(lib, dt, name):
    c, ops, tables, bias, ref, A, got, hi, P = single_case(lib, dt, name)
    check_single(got, ref, A, dt, name, P, ops.v)
    if name in ("narrow_tail_last", "beit_16x16", "tile_65"):
        _, hi2 = run(lib, dt, c, ops, tables, what=name)
        assert torch.equal(hi, hi2), f"{name}: two identical launches differ"


@pytest.mark.parametrize("name", ["wide", "beit_wide"])
def test_wide_and_narrow_forms_give_the_same_bits(lib, dt, name):
    c, ops, tables, bias, ref, A, got, hi, P = single_case(lib, dt, name)
    twin = rs.CASES[name + "_twin"]
    assert rs.launch_form(c)[1] == 2 and rs.launch_form(twin)[1] == 1
    got1, hi1 = run(lib, dt, twin, ops.take(1), tables, what=name + "_twin")
    assert torch.equal(hi[:1], hi1), f"{name}: image 0 of the wide launch differs from the narrow launch of image 0 alone"
    check_single(got1, ref[:1], A[:1], dt, name + "_twin", P[:1], ops.v[:1])


# ------------------------------------------------------------------------------------------------ three pass
X3 = [n for n, c in {**rs.PLAIN_CASES, **rs.BEIT_CASES}.items() if c["x3"] and not c["allow_split_kv"]]


@pytest.mark.parametrize("name", X3)
def test_three_pass_against_float64(lib, dt, name):
    c, ops, tables, bias, ref, A, got, hi, P = single_case(lib, dt, name)
    one = ops.hi_only(c)
    ref1, P1, A1 = rs.attention(one.q, one.k, one.v, bias)
    got1, _ = run(lib, dt, c, one, tables, x3=False, what=name + " single")
    check_single(got1, ref1, A1, dt, name + " on the hi planes", P1, one.v)
    check_x3(got, ref, A, ratio(got1, ref1, A1), dt, name)
    if name == "x3_linear":
        got2, hi2 = run(lib, dt, c, ops, tables, what=name)
        assert np.array_equal(got, got2), f"{name}: two identical launches differ"


# ------------------------------------------------------------------------------------------------ latency form
@pytest.mark.parametrize("name", ["split_40", "split_100", "split_325", "beit_split"])
def test_latency_form(lib, dt, name):
    c, ops, tables, bias, ref, A, got, hi, P = single_case(lib, dt, name)
    assert rs.launch_form(c)[4] == 1
    check_single(got, ref, A, dt, name, P, ops.v)
    whole, _ = run(lib, dt, c, ops, tables, what=name + " unsplit", allow_split_kv=0)
    check_single(whole, ref, A, dt, name + " unsplit", P, ops.v)
    check_single(got, whole, A, dt, name + " against the unsplit launch", P, ops.v, mul=2.0)
    _, hi2 = run(lib, dt, c, ops, tables, what=name)
    assert torch.equal(hi, hi2), f"{name}: two identical launches differ"


@pytest.mark.parametrize("name", ["unsplit_three_pass", "unsplit_big"])
def test_allow_split_kv_changes_nothing_where_the_rule_does_not_split(lib, dt, name):
    c, ops, tables, bias, ref, A, got, hi, P = single_case(lib, dt, name)
    assert rs.launch_form(c)[4] == 0
    got0, hi0 = run(lib, dt, c, ops, tables, what=name, allow_split_kv=0)
    assert np.array_equal(got, got0) and torch.equal(hi, hi0)
    if not c["x3"]:
        check_single(got, ref, A, dt, name, P, ops.v)


def test_a_query_does_not_depend_on_its_wave_partners_with_a_bias_table(lib, dt):
    c, ops, tables, bias, ref, A, got, hi, P = single_case(lib, dt, "beit_12x9")
    q2 = ops.q.copy()
    q2[:, :, 1::2] *= 7.0  # every other query becomes a very different row (much larger maxima)
    _, hi2 = run(lib, dt, c, Ops(q2, ops.k, ops.v, c, dt, seed=5), tables, what="beit_12x9 partners")
    assert torch.equal(hi[:, :, 0::2], hi2[:, :, 0::2])
    assert not torch.equal(hi[:, :, 1::2], hi2[:, :, 1::2])


# ------------------------------------------------------------------------------------------------ SwinV2 windows
_SWIN = {}


def plane_value(x, dt, lo):
    """the float64 value of the hi (+ lo) plane(s) of x"""
    t = t32(x)
    hi = t.to(dt)
    return (hi.double() + ((t - hi.float()).to(dt).double() if lo else 0.0)).numpy()


def swin_ops(name, dt):
    """operands and tables of a window case, built once per (case, format): q, k of rs.swin_operands, regions none / shifted / synthetic"""
    key = (name, dt)
    if key in _SWIN:
        return _SWIN[key]
    if name == "hard":
        c = rs.HARD_WINDOW
        q, k, lut = rs.swin_hard(np.random.default_rng(77))
        ls = rs.HARD_LS
        pairs = []
    else:
        c = rs.SWIN_CASES[name]
        q, k, lut, ls, pairs = rs.swin_operands(c, lambda x: plane_value(x, dt, bool(c["x3"])))
    g = np.random.default_rng(c["N"])
    v = g.standard_normal(q.shape)
    v = np.sign(v) * (0.25 + np.abs(v))  # (module docstring: no fp16-subnormal outputs on one-hot rows)
    ops = Ops(q, k, v, c, dt, seed=c["N"])
    tq, tk, rowmap0, _ = rs.swin_tables(c["gh"], c["gw"], c["wh"], c["ww"], 0, 0, c["npad"])
    _, _, rowmap_s, region_s = rs.swin_tables(c["gh"], c["gw"], c["wh"], c["ww"], c["wh"] // 2, c["ww"] // 2, c["npad"])
    regions = {"none": (rowmap0, None), "shift": (rowmap_s, region_s), "synthetic": (rowmap0, rs.synthetic_regions(g, c["win_nw"], c["N"]))}
    lut32 = lut.astype(np.float32)
    dev = dict(bias_lut=torch.from_numpy(lut32).cuda(), tq=torch.from_numpy(tq).cuda(), tk=torch.from_numpy(tk).cuda(),
               swin_ls=torch.from_numpy((ls * rs.LOG2E).astype(np.float32)).cuda())
    bias = lut32.astype(np.float64)[:, tq[:c["N"], None] - tk[None, :c["N"]]][None]
    _SWIN[key] = (c, ops, dev, bias, regions, {"pairs": pairs, "lut": lut32.astype(np.float64)})
    return _SWIN[key]


def swin_ref(entry, ops, kind):
    c, _, dev, bias, regions, refs = entry
    if (kind, id(ops)) not in refs:
        region = regions[kind][1]
        mask = None
        if region is not None:
            mask = np.tile(rs.region_mask(region), (c["B"] // c["win_nw"], 1, 1))[:, None]
        refs[(kind, id(ops))] = rs.attention(ops.q, ops.k, ops.v, bias, mask, score_mul=rs.LN2)
    return refs[(kind, id(ops))]


def region_rows(region, ld):
    """[nw, N] region ids -> device rows of stride ld (pad entries hold an id no token has)"""
    if region is None:
        return None
    full = np.full((region.shape[0], ld), 77, np.int32)
    full[:, :region.shape[1]] = region
    return torch.from_numpy(full).cuda()


def swin_run(lib, dt, entry, kind, ops=None, case=None, what="", **over):
    c, ops0, dev, bias, regions, _ = entry
    rowmap, region = regions[kind]
    tables = dict(dev, rowmap=torch.from_numpy(rowmap).cuda(), region=region_rows(region, (case or c)["region_ld"]))
    return run(lib, dt, case or c, ops or ops0, tables, rowmap=rowmap, what=f"{what} regions={kind}", **over)


def sub_windows(entry, n):
    """the first n windows of image 0 as a launch of their own: one image of 1 x n windows, their own rowmap, the same region rows"""
    c, ops, dev, bias, regions, _ = entry
    sub = dict(c, B=n, win_nw=n, images=1, gh=c["wh"], gw=n * c["ww"])
    _, _, rowmap, _ = rs.swin_tables(sub["gh"], sub["gw"], c["wh"], c["ww"], 0, 0, c["npad"])
    sregions = {kind: (rowmap, None if reg is None else np.ascontiguousarray(reg[:n])) for kind, (_, reg) in regions.items()}
    return (sub, ops.take(n), dev, bias, sregions, {})


@pytest.mark.parametrize("kind", ["none", "shift", "synthetic"])
@pytest.mark.parametrize("name", [n for n, c in rs.SWIN_CASES.items() if not c["x3"]] + ["hard"])
def test_window_attention_against_float64(lib, dt, name, kind):
    entry = swin_ops(name, dt)
    c, ops = entry[0], entry[1]
    ref, P, A = swin_ref(entry, ops, kind)
    got, hi = swin_run(lib, dt, entry, kind, what=name)
    check_single(got, ref, A, dt, f"{name} regions={kind}", P, ops.v)
    if name in rs.SWIN_TWINS:  # the 4-key runs and the re-strided table image are layouts, not arithmetic
        _, hi_r = swin_run(lib, dt, entry, kind, what=name + " no runs", bias_run4=0)
        assert torch.equal(hi, hi_r), f"{name} regions={kind}: bias_run4 = 1 and 0 differ"
        _, hi_s = swin_run(lib, dt, entry, kind, what=name + " own stride", bias_row=0, bias_ww=0)
        assert torch.equal(hi, hi_s), f"{name} regions={kind}: the re-strided and the plain table image differ"
    if name in ("win_8x8_wide", "win_12x12_wide", "win_16x20_wide"):  # the narrow form of the same windows, and a window alone in its batch
        n = 2 if name == "win_16x20_wide" else 8
        sub = sub_windows(entry, n)
        assert rs.launch_form(c)[1] == 2 and rs.launch_form(sub[0])[1] == 1
        _, hi_n = swin_run(lib, dt, sub, kind, what=name + " narrow twin")
        assert torch.equal(hi[:n], hi_n), f"{name} regions={kind}: the wide launch and the narrow launch of its first {n} windows differ"
    if name in ("win_7x7", "win_12x12"):
        sub = sub_windows(entry, 1)
        _, hi_1 = swin_run(lib, dt, sub, kind, what=name + " one window")
        assert torch.equal(hi[:1], hi_1), f"{name} regions={kind}: window 0 depends on the other windows of the batch"
        _, hi2 = swin_run(lib, dt, entry, kind, what=name)
        assert torch.equal(hi, hi2), f"{name}: two identical launches differ"


@pytest.mark.parametrize("kind", ["none", "shift", "synthetic"])
@pytest.mark.parametrize("name", [n for n, c in rs.SWIN_CASES.items() if c["x3"]])
def test_window_attention_three_pass(lib, dt, name, kind):
    entry = swin_ops(name, dt)
    c, ops = entry[0], entry[1]
    ref, P, A = swin_ref(entry, ops, kind)
    got, hi = swin_run(lib, dt, entry, kind, what=name)
    one = entry[5].setdefault("hi_only", ops.hi_only(c))
    ref1, P1, A1 = swin_ref(entry, one, kind)
    got1, _ = swin_run(lib, dt, entry, kind, ops=one, what=name + " single", x3=False)
    check_single(got1, ref1, A1, dt, f"{name} regions={kind} on the hi planes", P1, one.v)
    check_x3(got, ref, A, ratio(got1, ref1, A1), dt, f"{name} regions={kind}")
    if name in rs.SWIN_TWINS:
        _, hi_r = swin_run(lib, dt, entry, kind, what=name + " no runs", bias_run4=0)
        _, hi_s = swin_run(lib, dt, entry, kind, what=name + " own stride", bias_row=0, bias_ww=0)
        assert torch.equal(hi, hi_r) and torch.equal(hi, hi_s), f"{name} regions={kind}: the table layouts differ"


def test_a_window_query_does_not_depend_on_its_wave_partners(lib, dt):
    """inside the score contract: every other query is replaced by its own key exactly (the others keep their offset from theirs)"""
    entry = swin_ops("win_12x12", dt)
    c, ops, dev = entry[0], entry[1], entry[2]
    _, hi = swin_run(lib, dt, entry, "synthetic", what="partners")
    q2 = ops.q.copy()
    ls = f64(dev["swin_ls"])
    q2[:, :, 1::2] = ops.k[:, :, 1::2] * ls[None, :, None, None]
    _, hi2 = swin_run(lib, dt, entry, "synthetic", ops=Ops(q2, ops.k, ops.v, c, dt, seed=9), what="partners")
    assert torch.equal(hi[:, :, 0::2], hi2[:, :, 0::2])
    assert not torch.equal(hi[:, :, 1::2], hi2[:, :, 1::2])


# ------------------------------------------------------------------------------------------------ weights dump
def weights_case(lib, dt, what, c, ops, tables, P, lo):
    B, H, N = c["B"], c["heads"], c["N"]
    out = Out((B * H * N, N), torch.float32)
    planes = {n: t for n, t in ops.dev.items() if n[0] in "qk" and (lo or n.endswith("_hi"))}
    rc = launch(lib, "mdpt_debug_attn_weights_form", extra=(out,), **dict(ints(c), **planes, **tables))
    assert rc == 0, f"{what}: {lib.mdpt_last_error()}"
    assert out.guards_ok(), f"{what}: wrote into the guard rows"
    got = out.get().double().numpy().reshape(B, H, N, N)
    err = float(np.abs(got - P).max())
    print(f"MEASURE weights {fmt(dt)} {what}: max |got - P| = {err:.4e}, max |row sum - 1| = {float(np.abs(got.sum(-1) - 1).max()):.4e}")
    assert np.abs(got.sum(-1) - 1).max() <= N * 2.0 ** -23, f"{what}: rows do not sum to 1"
    m = MEASURED["weights"][fmt(dt)]
    assert err <= 4 * m, f"{what}: |got - P| = {err:.4e} above four times the recorded {m}"


@pytest.mark.parametrize("name", ["tile_65", "beit_12x9", "x3_tile_65", "beit_x3"])
def test_weights_dump_plain_and_table(lib, dt, name):
    c, ops, tables, bias, (ref, P, A), _ = plain_ops(name, dt)
    weights_case(lib, dt, name, c, ops, tables or {}, P, lo=bool(c["x3"]))


@pytest.mark.parametrize("kind", ["none", "shift", "synthetic"])
@pytest.mark.parametrize("name", ["win_7x7", "win_7x7_x3", "hard"])
def test_weights_dump_windows(lib, dt, name, kind):
    entry = swin_ops(name, dt)
    c, ops, dev, bias, regions, _ = entry
    rowmap, region = regions[kind]
    tables = dict(dev, rowmap=torch.from_numpy(rowmap).cuda(), region=region_rows(region, c["region_ld"]))
    weights_case(lib, dt, f"{name} regions={kind}", c, ops, tables, swin_ref(entry, ops, kind)[1], lo=bool(c["x3"]))


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("name", sorted(rs.REFUSALS))
def test_refused_launches_write_nothing(lib, dt, name):
    """every buffer is sized for the largest reading of the fields, so that a launch that slipped through would stay inside them"""
    bad = rs.REFUSALS[name]
    assert rs.launch_form(bad) == "refused"
    if bad["kind"] == "swin":
        entry = swin_ops("win_7x7", dt)
        c, ops, dev = entry[0], entry[1], entry[2]
        rowmap, region = entry[4]["shift"]
        tables = dict(dev, rowmap=torch.from_numpy(rowmap).cuda(), region=region_rows(region, c["region_ld"]))
        for field in ("bias_lut", "swin_ls", "rowmap"):
            if not bad[field]:
                tables[field] = None
        rows, ld = c["B"] * c["N"], c["F"]
    else:
        carrier = bad if name == "table_over_lds" else rs.plain_case(1, 9, 128)
        g = np.random.default_rng(3)
        shape = (carrier["B"], carrier["heads"], carrier["N"], 64)
        ops = Ops(g.standard_normal(shape) * 0.25, g.standard_normal(shape), g.standard_normal(shape), carrier, dt, seed=3)
        tables = {}
        if bad["kind"] == "beit":
            tq, tk, elen = rs.beit_tables(*bad["grid"], bad["npad"])
            tables = dict(bias_lut=torch.zeros(bad["heads"] * elen).cuda(), tq=torch.from_numpy(tq).cuda(), tk=torch.from_numpy(tk).cuda())
        rows, ld = carrier["B"] * carrier["npad"], max(carrier["F"], bad["F"])
    o_hi = Out((rows, ld), dt)
    planes = {n: t for n, t in ops.dev.items() if n.endswith("_hi")}
    rc = launch(lib, **dict(ints(bad), **planes, **tables, out_hi=o_hi))
    assert rc == INVALID, f"{name}: returned {rc}, not hipErrorInvalidValue"
    assert o_hi.untouched(), f"{name}: a refused launch wrote to the output"
