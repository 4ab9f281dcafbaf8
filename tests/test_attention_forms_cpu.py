"""The float64 restatements of tests/attention_restate.py against independent torch formulations, the coverage of the case table of
tests/test_gpu_attention_forms.py (all 14 attn_kernel instantiations are reached, nothing is refused by accident) and the score contract of
the fixed-reference window form on the operands that test feeds the kernel. Runs without a GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import attention_restate as rs


def rng(seed):
    return np.random.default_rng(seed)


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("score_mul", [1.0, rs.LN2])
def test_attention_is_sdpa_with_an_additive_mask(score_mul):
    g = rng(1)
    q, k, v = (g.standard_normal((2, 3, 37, 32)) for _ in range(3))
    bias = g.standard_normal((1, 3, 37, 37)) * 2
    mask = np.where(g.random((2, 1, 37, 37)) < 0.3, rs.MASK, 0.0)
    out, p, a = rs.attention(q, k, v, bias, mask, score_mul)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    ref = F.scaled_dot_product_attention(t(q), t(k), t(v), attn_mask=t(bias + mask), scale=score_mul)
    assert np.abs(out - ref.numpy()).max() < 1e-12
    assert np.abs(p.sum(-1) - 1).max() < 1e-13 and np.abs(a - p @ np.abs(v)).max() == 0.0
    out0, _, _ = rs.attention(q, k, v)
    assert np.abs(out0 - F.scaled_dot_product_attention(t(q), t(k), t(v), scale=1.0).numpy()).max() < 1e-12


# ------------------------------------------------------------------------------------------------ SwinV2 window map
def _partition(img, wh, ww):
    gh, gw = img.shape
    return img.view(gh // wh, wh, gw // ww, ww).permute(0, 2, 1, 3).reshape(-1, wh * ww)


@pytest.mark.parametrize("gh,gw,wh,ww,sh,sw", [(14, 14, 7, 7, 3, 3), (12, 20, 6, 10, 3, 5), (24, 48, 24, 24, 12, 12), (16, 16, 8, 8, 0, 0),
                                              (8, 16, 8, 8, 0, 4), (64, 160, 16, 20, 8, 10)])
def test_window_map_is_roll_then_partition(gh, gw, wh, ww, sh, sw):
    tq, tk, rowmap, region = rs.swin_tables(gh, gw, wh, ww, sh, sw, npad=(wh * ww + 7) // 8 * 8)
    ids = torch.arange(gh * gw).view(gh, gw)
    assert torch.equal(_partition(torch.roll(ids, shifts=(-sh, -sw), dims=(0, 1)), wh, ww).flatten(), torch.from_numpy(rowmap).long())
    assert sorted(rowmap.tolist()) == list(range(gh * gw))  # a permutation: every image row is written once
    if sh or sw:  # the reference's make_shift_mask: nine slices, in its order, on the rolled image
        img, cnt = torch.zeros(gh, gw), 0
        for hs in (slice(0, -wh), slice(-wh, -sh), slice(-sh, None)):
            for ws in (slice(0, -ww), slice(-ww, -sw), slice(-sw, None)):
                img[hs, ws] = cnt
                cnt += 1
        mw = _partition(img, wh, ww)
        diff = mw.unsqueeze(1) - mw.unsqueeze(2)
        want = diff.masked_fill(diff != 0, -100.0).masked_fill(diff == 0, 0.0)
        assert np.array_equal(rs.region_mask(region), want.numpy())
    # the relative-position index of the reference: (dy + wh - 1)(2 ww - 1) + dx + ww - 1
    wa = wh * ww
    for i in (0, 1, ww, wa - 1):
        for j in (0, ww - 1, wa // 2, wa - 1):
            (yi, xi), (yj, xj) = divmod(i, ww), divmod(j, ww)
            assert tq[i] - tk[j] == (yi - yj + wh - 1) * (2 * ww - 1) + xi - xj + ww - 1
    assert (tq[wa:] == tq[wa - 1]).all() and (tk[wa:] == tk[wa - 1]).all()
    assert 0 <= (tq[:, None] - tk[None, :]).min() and (tq[:, None] - tk[None, :]).max() < (2 * wh - 1) * (2 * ww - 1)


# ------------------------------------------------------------------------------------------------ BEiT tables
@pytest.mark.parametrize("gh,gw", [(5, 7), (12, 9), (16, 16), (15, 16)])
def test_beit_extended_table_is_the_reference_index_matrix(gh, gw):
    N, rw = gh * gw + 1, 2 * gw - 1
    R = (2 * gh - 1) * rw
    index = np.zeros((N, N), np.int64)
    for qi in range(N):
        for ki in range(N):
            if qi == 0 and ki == 0:
                index[qi, ki] = R + 2
            elif qi == 0:
                index[qi, ki] = R
            elif ki == 0:
                index[qi, ki] = R + 1
            else:
                (yq, xq), (yk, xk) = divmod(qi - 1, gw), divmod(ki - 1, gw)
                index[qi, ki] = (yq - yk + gh - 1) * rw + xq - xk + gw - 1
    table = rng(gh * 100 + gw).standard_normal(R + 3)
    npad = (N + 7) // 8 * 8
    tq, tk, elen = rs.beit_tables(gh, gw, npad)
    ext = rs.beit_extend(table, gh, gw)
    assert len(ext) == elen == 2 * R + 2 * ((gh - 1) * rw + gw - 1) + 2
    idx = tq[:, None].astype(np.int64) - tk[None, :]
    assert idx.min() >= 0 and idx.max() < elen  # pad entries included: in range
    assert np.array_equal(ext[idx[:N, :N]], table[index])
    assert (tq[N:] == tq[1]).all() and (tk[N:] == tk[1]).all()


# ------------------------------------------------------------------------------------------------ the case table
def test_case_table_reaches_every_instantiation_and_nothing_is_refused_by_accident():
    launches = list(rs.CASES.values()) + [t for pair in rs.SWIN_TWINS.values() for t in pair]
    forms = {rs.launch_form(c) for c in launches}
    assert "refused" not in forms
    assert forms == rs.ALL_FORMS and len(rs.ALL_FORMS) == 14
    for name, c in rs.REFUSALS.items():
        assert rs.launch_form(c) == "refused", name
    # the paths the table promises
    f = lambda n: rs.launch_form(rs.CASES[n])
    assert f("wide") == (0, 2, 0, 64, 0, 0) and f("wide_twin") == (0, 1, 0, 64, 0, 0)
    assert f("beit_wide") == (0, 2, 1, 64, 0, 0) and f("beit_wide_twin") == (0, 1, 1, 64, 0, 0) and f("beit_split") == (0, 1, 1, 64, 1, 0)
    assert f("win_12x12_wide") == (0, 2, 2, 32, 0, 1) and f("win_12x12") == (0, 1, 2, 32, 0, 1)
    assert rs.CASES["win_6x10"]["region_ld"] == rs.CASES["win_6x10"]["N"] + 8
    assert f("win_8x8_wide") == (0, 2, 2, 32, 0, 1) and f("win_8x8_narrow") == (0, 1, 2, 32, 0, 1) and f("win_16x20_wide") == (0, 2, 2, 32, 0, 1)
    assert f("win_7x7") == f("win_6x10") == (0, 1, 2, 32, 0, 0) and f("win_12x12_x3") == (1, 1, 2, 32, 0, 1)
    assert all(f(n)[4] == 1 for n in ("split_40", "split_100", "split_325")) and f("unsplit_big")[4] == 0 and f("unsplit_three_pass")[4] == 0
    assert rs.CASES["narrow_linear"]["B"] * rs.CASES["narrow_linear"]["heads"] % 8 != 0
    for n in ("narrow_tail_last", "beit_16x16", "win_16x20_wide"):  # tail_last: the last q-tile holds at most one wave's queries
        c, form = rs.CASES[n], f(n)
        qpw = 32 * form[1]
        assert c["B"] * c["heads"] % 8 == 0 and c["npad"] > 4 * qpw and c["npad"] % (4 * qpw) <= qpw and c["npad"] % (4 * qpw) > 0, n
    c = rs.CASES["win_12x12"]
    assert c["bias_row"] == 23 and c["bias_row"] + ((c["bias_ww"] - c["bias_row"]) % 32) == 44 and c["out_ld"] == c["F"] + 32


# ------------------------------------------------------------------------------------------------ the fixed-reference contract
def _rounded(x, dtype, lo=False):
    """the value of the hi (+ lo) plane(s) of x"""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    hi = t.to(dtype)
    return (hi.double() + ((t - hi.float()).to(dtype).double() if lo else 0.0)).numpy()


def _check_contract(q, k, lut, ls_nat, tq, tk, N, dtype, what):
    """float64 on the rounded planes: every score (log2 units, bias included) <= M_h, every own-key score >= ls_h (1 - 2^-7)"""
    ls = (ls_nat * rs.LOG2E).astype(np.float32).astype(np.float64)  # what the kernel is handed as swin_ls
    qr, kr = _rounded(q, dtype), _rounded(k, dtype)
    bias = lut[:, tq[:N, None] - tk[None, :N]] * rs.LOG2E  # [heads, N, N]
    for h in range(q.shape[1]):
        dots = qr[:, h] @ np.swapaxes(kr[:, h], -1, -2)
        s = dots + bias[h]
        assert s.max() <= rs.fixref_bound(ls[h]), f"{what} head {h}: score {s.max()} above M_h {rs.fixref_bound(ls[h])}"
        own = np.diagonal(dots, axis1=-2, axis2=-1)
        assert own.min() >= ls[h] * (1 - 2.0 ** -7), f"{what} head {h}: own-key score {own.min()} below {ls[h] * (1 - 2.0 ** -7)}"
        assert lut[h].min() >= 0.0 and lut[h].max() < 16.0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", sorted(rs.SWIN_CASES))
def test_window_operands_keep_the_fixed_reference_contract(name, dtype):
    c = rs.SWIN_CASES[name]
    rnd = lambda x: _rounded(x, dtype, lo=bool(c["x3"]))
    q, k, lut, ls, pairs = rs.swin_operands(c, rnd)
    tq, tk, _, _ = rs.swin_tables(c["gh"], c["gw"], c["wh"], c["ww"], 0, 0, c["npad"])
    _check_contract(q, k, lut, ls, tq, tk, c["N"], dtype, name)
    assert ls.min() == 1.0 and ls.max() == 100.0
    # the threshold rows: in every multi-tile window, in the heads with a logit scale of 16 or more, on the values the planes hold
    if c["N"] > 64:
        assert {p[0] for p in pairs} >= {h for h in range(c["heads"]) if ls[h] >= 16.0}, pairs
        for (h, qi, ka, kb), (under, over) in zip(pairs, rs.swin_threshold_gaps(c, rnd(q), rnd(k), lut, pairs)):
            assert qi < 64 <= ka < 128 and kb >= (c["N"] - 1) // 64 * 64
            assert -0.5 < under < 0 < over < 0.5, f"{name} head {h}: ka {under:+.3f}, kb {over:+.3f} from the threshold"
        assert "win_12x12" not in name or all(c["N"] % 64 and p[3] >= 128 for p in pairs)  # kb in the partial last tile
    else:
        assert pairs == []


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_hard_window_rows_keep_the_fixed_reference_contract(dtype):
    c = rs.HARD_WINDOW
    q, k, lut = rs.swin_hard(rng(77))
    tq, tk, _, _ = rs.swin_tables(c["gh"], c["gw"], c["wh"], c["ww"], 0, 0, c["npad"])
    _check_contract(q, k, lut, rs.HARD_LS, tq, tk, c["N"], dtype, "hard rows")
    assert lut[0].max() < 0.25 and lut[1].min() >= 15.75
