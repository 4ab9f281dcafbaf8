"""Plain numpy float64 restatements of what the fused attention (csrc/attention.hip, csrc/mdpt_kernels.h AttnParams) computes and of the index
tables it is handed, written from the comments of the kernels that produce them and from the reference's formulas - not from the kernel code:

  attention()        softmax(score_mul * q k^T + bias + mask) v, with the probabilities P and A = P |v| (the scale of the error bounds)
  beit_tables()      tq, tk, elen and the extended-table layout of a gh x gw grid with a cls token (comment of beit_relpos_body, csrc/ew_tokens.inc)
  swin_tables()      tq, tk, rowmap, region of a (grid, window, shift) (comment of swin_window_map_kernel, csrc/swin.hip)
  launch_form()      the launcher's selection rule: which of the 14 attn_kernel instantiations a launch resolves to, or "refused"

tests/test_attention_forms_cpu.py proves each against an independent torch formulation; tests/test_gpu_attention_forms.py compares the kernels
with them. CASES is the case table both walk."""
import math

import numpy as np

F64 = np.float64
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
MASK = -100.0  # the shifted-window mask value of the reference (natural units)


def attention(q, k, v, bias=None, mask=None, score_mul=1.0):
    """q, k, v [..., N, d]; bias, mask broadcastable to [..., N, N] -> (out, P, A): out = P v, P = softmax(score_mul q k^T + bias + mask),
    A = P |v|."""
    q, k, v = (np.asarray(x, F64) for x in (q, k, v))
    s = score_mul * (q @ np.swapaxes(k, -1, -2))
    if bias is not None:
        s = s + np.asarray(bias, F64)
    if mask is not None:
        s = s + np.asarray(mask, F64)
    s = s - s.max(axis=-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(axis=-1, keepdims=True)
    return p @ v, p, p @ np.abs(v)


# ---- BEiT: bias(q, k) = ext[tq[q] - tk[k]]
def beit_tables(gh, gw, npad=None):
    """Token 0 is cls, token 1 + y * gw + x the patch (y, x). With rw = 2 gw - 1, R = (2 gh - 1) rw, T = (gh - 1) rw + gw - 1:
    tq = (y + gh - 1) rw + x + gw - 1, tk = y rw + x for patches (their difference is the usual relative-position index, in [0, R));
    tq[cls] = R + T, tk[cls] = -(R + T + 1). Pad entries [N, npad) take the values of token 1. Returns tq, tk, elen = 2 R + 2 T + 2."""
    rw = 2 * gw - 1
    R, T = (2 * gh - 1) * rw, (gh - 1) * rw + gw - 1
    N = gh * gw + 1
    npad = N if npad is None else npad
    tq, tk = np.zeros(npad, np.int32), np.zeros(npad, np.int32)
    for t in range(npad):
        tt = t if t < N else 1
        if tt == 0:
            tq[t], tk[t] = R + T, -(R + T + 1)
        else:
            y, x = divmod(tt - 1, gw)
            tq[t], tk[t] = (y + gh - 1) * rw + x + gw - 1, y * rw + x
    return tq, tk, 2 * R + 2 * T + 2


def beit_extend(table, gh, gw):
    """The extended table of one head from the reference's [R + 3] table (R token-token entries, then cls->token, token->cls, cls->cls):
    [0, R) as they are, [R, R + T] = cls->token, [R + T + 1, 2 R + T] = token->cls, [2 R + 2 T + 1] = cls->cls, 0 elsewhere."""
    rw = 2 * gw - 1
    R, T = (2 * gh - 1) * rw, (gh - 1) * rw + gw - 1
    table = np.asarray(table, F64)
    ext = np.zeros(2 * R + 2 * T + 2, F64)
    ext[:R] = table[:R]
    ext[R:R + T + 1] = table[R]
    ext[R + T + 1:2 * R + T + 1] = table[R + 1]
    ext[2 * R + 2 * T + 1] = table[R + 2]
    return ext


# ---- SwinV2 windows
def swin_tables(gh, gw, wh, ww, sh, sw, npad=None):
    """Windows are numbered wy * nWx + wx, tokens inside a window iy * ww + ix. The reference rolls the image by (-sh, -sw) before partitioning:
    the window token at rolled position (y', x') is image token ((y' + sh) mod gh, (x' + sw) mod gw). region = 3 * hslice + wslice of the rolled
    position, slices [0, g - w), [g - w, g - s), [g - s, g); a zero shift in a dimension puts everything into that dimension's last slice.
    tq = (iy + wh - 1)(2 ww - 1) + ix + ww - 1, tk = iy (2 ww - 1) + ix; pad entries take the last token's. Returns tq, tk [npad],
    rowmap [nw * wa], region [nw, wa]."""
    wa, nwx = wh * ww, gw // ww
    nw = (gh // wh) * nwx
    npad = wa if npad is None else npad
    tq, tk = np.zeros(npad, np.int32), np.zeros(npad, np.int32)
    for t in range(npad):
        iy, ix = divmod(min(t, wa - 1), ww)
        tq[t], tk[t] = (iy + wh - 1) * (2 * ww - 1) + ix + ww - 1, iy * (2 * ww - 1) + ix
    rowmap, region = np.zeros(nw * wa, np.int32), np.zeros((nw, wa), np.int32)
    for w in range(nw):
        wy, wx = divmod(w, nwx)
        for i in range(wa):
            iy, ix = divmod(i, ww)
            yr, xr = wy * wh + iy, wx * ww + ix
            rowmap[w * wa + i] = ((yr + sh) % gh) * gw + (xr + sw) % gw
            rh = 2 if sh == 0 else (0 if yr < gh - wh else (1 if yr < gh - sh else 2))
            rw_ = 2 if sw == 0 else (0 if xr < gw - ww else (1 if xr < gw - sw else 2))
            region[w, i] = 3 * rh + rw_
    return tq, tk, rowmap, region


def region_mask(region):
    """[nw, wa] region ids -> [nw, wa, wa] additive mask: 0 inside a region, -100 across."""
    region = np.asarray(region)
    return np.where(region[:, :, None] != region[:, None, :], MASK, 0.0)


def fixref_bound(ls_h):
    """M_h of the bf16 window form (log2 units; ls_h = logit scale * log2 e as packed)."""
    return ls_h * (1.0 + 2.0 ** -6) + 16.0 * LOG2E


# ---- the launcher's selection rule
def _rup(x, m):
    return (x + m - 1) // m * m


def launch_form(case):
    """case: a dict of the AttnParams fields (pointers as booleans: bias_lut, rowmap, swin_ls) -> (X3, QB, MODE, HD, SPLIT, RUN4) or "refused".
    The rule is the same in both operand formats."""
    g = lambda n, d=0: case.get(n, d)
    hd = g("head_dim") or 64
    B, heads, N, npad, npadv, F = g("B"), g("heads"), g("N"), g("npad"), g("npadv"), g("F")
    if hd not in (64, 32) or F != heads * hd or npadv % 64 or npadv < _rup(N, 64) or npad < N:
        return "refused"
    swin, bias, x3 = bool(g("rowmap")), bool(g("bias_lut")), bool(g("x3"))
    if swin and (hd != 32 or not bias or not g("swin_ls") or g("win_nw") <= 0 or B % g("win_nw")):
        return "refused"
    if not swin and hd != 64:
        return "refused"
    blocks256 = _rup(npad, 256) // 256 * heads * B
    fills = hd == 32 or _rup(N, 256) * 100 <= N * 108
    wide = not x3 and blocks256 >= 512 and fills
    elen, row, ww = g("bias_elen"), g("bias_row"), g("bias_ww")
    restr = swin and bool(g("bias_run4")) and row > 0 and ww > 0 and elen % row == 0
    entries = (elen // row) * (row + ((ww - row) % 32)) if restr else elen
    extra = entries * 4 + _rup(N, 64) * 4 * (2 if swin else 1) if bias else 0
    ring = 2 * 2 * (2 if x3 else 1) * 64 * hd * 2
    if ring + extra > 160 * 1024:
        return "refused"
    blocks32 = _rup(npad, 32) // 32 * heads * B
    if g("allow_split_kv") and not swin and not x3 and blocks32 <= 320 and 4 * ring + extra <= 160 * 1024:
        return (0, 1, 1 if bias else 0, 64, 1, 0)
    mode = 2 if swin else (1 if bias else 0)
    return (int(x3), 2 if wide else 1, mode, hd, 0, 1 if (mode == 2 and g("bias_run4")) else 0)


ALL_FORMS = frozenset(
    [(0, qb, m, hd, 0, 0) for qb in (1, 2) for m, hd in ((0, 64), (1, 64), (2, 32))] + [(1, 1, m, hd, 0, 0) for m, hd in ((0, 64), (1, 64), (2, 32))]
    + [(0, 1, 2, 32, 0, 1), (0, 2, 2, 32, 0, 1), (1, 1, 2, 32, 0, 1)] + [(0, 1, 0, 64, 1, 0), (0, 1, 1, 64, 1, 0)])


# ---- the case table of tests/test_gpu_attention_forms.py
def plain_case(B, heads, N, x3=0, split=0, grid=None):
    """head dim 64; grid = (gh, gw): BEiT bias table, N = gh * gw + 1"""
    if grid:
        N = grid[0] * grid[1] + 1
    c = dict(kind="beit" if grid else "plain", B=B, heads=heads, N=N, npad=_rup(N, 8), npadv=_rup(N, 64), F=heads * 64, x3=x3, allow_split_kv=split,
             grid=grid)
    if grid:
        c.update(bias_lut=True, bias_elen=beit_tables(*grid)[2])
    return c


def swin_case(wh, ww, images=2, nwy=2, nwx=2, heads=4, x3=0, run4=None, restride=True, out_pad=0, region_pad=0):
    """head dim 32; images x (nwy x nwx) windows of wh x ww tokens on a (nwy wh) x (nwx ww) grid. run4 None: the model's rule."""
    wa = wh * ww
    if run4 is None:
        run4 = int(ww % 4 == 0 and wa % 4 == 0)
    return dict(kind="swin", B=images * nwy * nwx, heads=heads, N=wa, npad=_rup(wa, 8), npadv=_rup(wa, 64), F=heads * 32, x3=x3, head_dim=32,
                bias_lut=True, bias_elen=(2 * wh - 1) * (2 * ww - 1), rowmap=True, swin_ls=True, win_nw=nwy * nwx, region_ld=wa + region_pad, bias_run4=run4,
                bias_row=2 * ww - 1 if restride else 0, bias_ww=ww if restride else 0, out_ld=heads * 32 + out_pad if out_pad else 0,
                wh=wh, ww=ww, gh=nwy * wh, gw=nwx * ww, images=images)


PLAIN_CASES = {
    "narrow_linear": plain_case(1, 3, 150),
    "narrow_tail_last": plain_case(1, 8, 150),
    "wide": plain_case(32, 16, 250),
    "wide_twin": plain_case(1, 16, 250),
    "tile_40": plain_case(1, 8, 40),
    "tile_64": plain_case(1, 8, 64),
    "tile_65": plain_case(1, 8, 65),
    "x3_linear": plain_case(1, 3, 150, x3=1),
    "x3_tail_last": plain_case(1, 8, 150, x3=1),
    "x3_tile_40": plain_case(1, 8, 40, x3=1),
    "x3_tile_64": plain_case(1, 8, 64, x3=1),
    "x3_tile_65": plain_case(1, 8, 65, x3=1),
    "split_40": plain_case(1, 6, 40, split=1),
    "split_100": plain_case(1, 6, 100, split=1),
    "split_325": plain_case(1, 6, 325, split=1),
    "unsplit_three_pass": plain_case(1, 3, 150, x3=1, split=1),  # allow_split_kv set, but the rule does not split these two
    "unsplit_big": plain_case(5, 16, 150, split=1),
}
BEIT_CASES = {
    "beit_5x7": plain_case(1, 8, 0, grid=(5, 7)),
    "beit_12x9": plain_case(1, 8, 0, grid=(12, 9)),
    "beit_16x16": plain_case(1, 8, 0, grid=(16, 16)),
    "beit_wide": plain_case(32, 16, 0, grid=(15, 16)),
    "beit_wide_twin": plain_case(1, 16, 0, grid=(15, 16)),
    "beit_x3": plain_case(1, 8, 0, grid=(12, 9), x3=1),
    "beit_split": plain_case(1, 4, 0, grid=(12, 9), split=1),
}
SWIN_CASES = {
    "win_7x7": swin_case(7, 7),
    "win_6x10": swin_case(6, 10, region_pad=8),  # region rows of stride N + 8
    "win_8x8_wide": swin_case(8, 8, nwy=8, nwx=8),
    "win_8x8_narrow": swin_case(8, 8),
    "win_12x12": swin_case(12, 12, out_pad=32),
    "win_12x12_wide": swin_case(12, 12, nwy=8, nwx=8),  # wide with a partial last key tile
    "win_16x20_wide": swin_case(16, 20, nwy=4, nwx=8),
    "win_24x24": swin_case(24, 24, nwy=1, nwx=2, heads=2),
    "win_8x8_x3": swin_case(8, 8, x3=1),
    "win_7x7_x3": swin_case(7, 7, x3=1),
    "win_12x12_x3": swin_case(12, 12, x3=1),
}
CASES = {**PLAIN_CASES, **BEIT_CASES, **SWIN_CASES}
# twins that must give the same bits: the 4-key runs switched off, the table's own row stride
SWIN_TWINS = {n: (dict(c, bias_run4=0), dict(c, bias_row=0, bias_ww=0)) for n, c in SWIN_CASES.items() if c["bias_run4"]}

_BASE, _WIN = PLAIN_CASES["tile_40"], SWIN_CASES["win_7x7"]
REFUSALS = {
    "npadv_not_64": dict(_BASE, npadv=72),
    "npadv_short": dict(plain_case(1, 8, 100), npadv=64),
    "npad_short": dict(_BASE, npad=32),
    "F_mismatch": dict(_BASE, F=_BASE["F"] + 64),
    "head_dim_48": dict(_BASE, head_dim=48, F=8 * 48),
    "rowmap_no_lut": dict(_WIN, bias_lut=False),
    "rowmap_no_ls": dict(_WIN, swin_ls=False),
    "B_not_windows": dict(_WIN, win_nw=3),
    "hd32_no_rowmap": dict(_WIN, rowmap=False),
    "table_over_lds": plain_case(1, 1, 0, grid=(64, 64)),
}


# ---- operands of the window cases: inside the FIXREF contract by construction (test_attention_forms_cpu.py checks it on the rounded planes)
def swin_logit_scales(heads):
    """per head, natural units: 1 .. 100 geometrically, the last exactly 100"""
    return np.array([100.0 ** (h / max(heads - 1, 1)) for h in range(heads)])


def swin_qk(rng, B, heads, N, ls):
    """Unit-vector keys drawn around a few centres per (window, head) (so that several keys of a row score alike even at logit scale 100) and
    queries within cos >= 1 - 2^-9 of their own key, times ls * log2 e. Returns q, k [B, heads, N, 32] float64 (unrounded)."""
    nc = max(2, N // 6)
    cen = rng.standard_normal((B, heads, nc, 32))
    k = np.take_along_axis(cen, rng.integers(0, nc, (B, heads, N, 1)).repeat(32, -1), 2) / math.sqrt(32) + 0.15 * _unit(rng.standard_normal((B, heads, N, 32)))
    k = _unit(k)
    q = _unit(k + 0.05 * _unit(rng.standard_normal((B, heads, N, 32))))
    return q * (ls * LOG2E)[None, :, None, None], k


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def swin_lut(rng, heads, elen, lo=0.0, hi=16.0):
    """distinct random table entries per head inside [lo, hi) (the reference's table is 16 sigmoid(.) < 16), fp32-exact"""
    return rng.uniform(lo, hi, (heads, elen)).astype(np.float32).clip(lo, np.nextafter(np.float32(hi), np.float32(0))).astype(F64)


def synthetic_regions(rng, nw, wa):
    """region ids 0 .. 3 at random, with two singleton regions per window (tokens 2 and wa - 1)"""
    reg = rng.integers(0, 4, (nw, wa)).astype(np.int32)
    reg[:, 2], reg[:, wa - 1] = 100, 101
    return reg


HARD_LS = np.array([100.0, 100.0, 1.0, 30.0])  # natural units, per head
HARD_WINDOW = swin_case(8, 8, images=1, nwy=1, nwx=2)


def swin_hard(rng):
    """The rows at the ends of the fixed-reference range (8 x 8 window, 2 windows, 4 heads; head 0: table entries in [0, 0.25), head 1: in
    [15.75, 16), both at logit scale 100). Window 0: every key is -e except key 1 = +e, queries = their own keys: query 1 sees only itself (the
    smallest denominator), every other query all keys but one aligned (with head 1: the largest). Window 1: all keys within a narrow cone, so
    that under the synthetic regions the masked keys of a singleton-region query score as high as its own. Returns q, k (unrounded), lut."""
    c = HARD_WINDOW
    B, heads, N = c["B"], c["heads"], c["N"]
    ls = HARD_LS * LOG2E
    e = _unit(rng.standard_normal((heads, 1, 32)))
    k = np.zeros((B, heads, N, 32))
    k[0] = -e
    k[0, :, 1] = e[:, 0]
    k[1] = _unit(_unit(rng.standard_normal((heads, 1, 32))) + 0.02 * _unit(rng.standard_normal((heads, N, 32))))
    q = k * ls[None, :, None, None]
    lut = swin_lut(rng, heads, c["bias_elen"])
    lut[0] = swin_lut(rng, 1, c["bias_elen"], 0.0, 0.25)[0]
    lut[1] = swin_lut(rng, 1, c["bias_elen"], 15.75, 16.0)[0]
    return q, k, lut


DEFER = 5.5  # kDeferMax of csrc/attention.hip (natural units; the window forms compare in log2 units)


def defer_walk(s_row, upto, defer=DEFER):
    """the reference point of a row after the key tiles before `upto` (it starts at the first tile's maximum and moves to a tile's maximum only
    when that exceeds it by more than `defer`)"""
    m = -1.0e30
    for t0 in range(0, upto, 64):
        mx = s_row[t0:min(t0 + 64, upto)].max()
        if mx > m + defer:
            m = mx
    return m


def swin_threshold_rows(case, q, k, lut, ls, rnd):
    """The rows at the deferred-maximum threshold of the window forms that track a maximum (the fp16 build), inside the score contract: in window 0
    of every head that leaves room, a query qi of the first key tile gets two copies of its own key, ka in the second tile and kb in the last
    one (the partial one where N is no multiple of 64), and the two table entries lut[tq[qi] - tk[ka]], lut[tq[qi] - tk[kb]] are set from the
    float64 scores of the rounded operands (rnd) so that ka scores 0.25 (log2 units) under m + DEFER log2 e and kb 0.25 over it, m = the
    row's maximum over the first tile. The own-key entry of the table is quartered first. A head has room when both entries land in [0, 16), no other later
    key comes within 0.5 of the threshold and kb stays under M_h: with random table entries up to 16 that needs a logit scale of about 16 or
    more. q, k, lut are changed in place; returns [(head, qi, ka, kb)]."""
    N, heads = case["N"], case["heads"]
    last = (N - 1) // 64 * 64
    if last == 0:
        return []
    tq, tk, _, _ = swin_tables(case["wh"], case["ww"], case["wh"], case["ww"], 0, 0)
    thr, pairs = DEFER * LOG2E, []
    for h in range(heads):
        lsh = float(np.float32(ls[h] * LOG2E))
        lut[h, tq[0] - tk[0]] = np.float32(lut[h, tq[0] - tk[0]] / 4)
        for qi in range(2, 64):
            ka, kb = 64 + qi % 48, N - 1 - qi % 8
            kk = k[0, h].copy()
            kk[ka] = kk[kb] = k[0, h, qi]
            dots = rnd(kk) @ rnd(q[0, h, qi])
            s = dots + lut[h, tq[qi] - tk[:N]] * LOG2E
            m = s[:64].max()
            others = np.delete(s[64:], [ka - 64, kb - 64])
            la, lb = np.float32((m + thr - 0.25 - dots[ka]) / LOG2E), np.float32((m + thr + 0.25 - dots[kb]) / LOG2E)
            if others.max() <= m + thr - 0.5 and 0 <= la < 15.99 and 0 <= lb < 15.99 and m + thr + 0.3 <= fixref_bound(lsh):
                k[0, h, ka] = k[0, h, kb] = k[0, h, qi]
                q[0, h, ka] = q[0, h, kb] = q[0, h, qi]
                lut[h, tq[qi] - tk[ka]], lut[h, tq[qi] - tk[kb]] = la, lb
                pairs.append((h, qi, ka, kb))
                break
    return pairs


def swin_threshold_gaps(case, qv, kv, lut, pairs):
    """(log2 units) how far ka and kb of each pair sit from the threshold on the operand values qv, kv [B, heads, N, 32] the kernel is handed:
    ka against the reference point after the first tile, kb against the one before the last tile"""
    N = case["N"]
    last = (N - 1) // 64 * 64
    tq, tk, _, _ = swin_tables(case["wh"], case["ww"], case["wh"], case["ww"], 0, 0)
    out = []
    for h, qi, ka, kb in pairs:
        s = kv[0, h] @ qv[0, h, qi] + lut[h, tq[qi] - tk[:N]] * LOG2E
        m1 = defer_walk(s, 64, DEFER * LOG2E)
        assert s[64:128].argmax() == ka - 64 and s[last:].argmax() == kb - last
        out.append((s[ka] - (m1 + DEFER * LOG2E), s[kb] - (defer_walk(s, last, DEFER * LOG2E) + DEFER * LOG2E)))
    return out


def swin_operands(case, rnd=None, seed=None):
    """q, k [B, heads, N, 32] (unrounded), lut [heads, elen], logit scales (natural units) of a window case and, with rnd (the rounding of the
    operand planes the case runs on), the threshold rows of swin_threshold_rows: the same for every test that runs it"""
    g = np.random.default_rng(case["wh"] * 1000 + case["ww"] * 10 + case["B"] if seed is None else seed)
    ls = swin_logit_scales(case["heads"])
    q, k = swin_qk(g, case["B"], case["heads"], case["N"], ls)
    lut = swin_lut(g, case["heads"], case["bias_elen"])
    pairs = swin_threshold_rows(case, q, k, lut, ls, rnd) if rnd is not None else []
    return q, k, lut, ls, pairs
