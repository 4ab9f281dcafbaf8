"""The float64 restatements of the GEMM forms (tests/gemm_forms_restate.py) against INDEPENDENT torch float64 formulations of the same operations,
on the shapes tests/test_gpu_gemm_forms.py runs: the references are proven here, without a GPU, before a kernel is compared with them."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import gemm_forms_restate as rs

TOL = 1e-12  # float64 against float64 in another summation order, values of order 1


def _rand(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape)


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _close(got, want):
    want = want.numpy() if isinstance(want, torch.Tensor) else want
    assert got.shape == want.shape, (got.shape, want.shape)
    assert float(np.abs(got - want).max()) <= TOL * max(1.0, float(np.abs(want).max()))


@pytest.mark.parametrize("hw", [(9, 11), (8, 10)])
@pytest.mark.parametrize("cin", [64, 128])
@pytest.mark.parametrize("stride", [1, 2])
def test_conv_rows_and_packed_weights_are_a_padded_strided_convolution(hw, cin, stride):
    B, cout = 2, 64
    x, w, b = _rand(1, B, *hw, cin), _rand(2, cout, cin, 3, 3), _rand(3, cout)
    got = rs.generic(rs.product(rs.conv3_rows(x, stride), rs.pack_conv3(w)), b)
    want = F.conv2d(_t(x).permute(0, 3, 1, 2), _t(w), _t(b), stride=stride, padding=1).permute(0, 2, 3, 1)
    assert want.shape[1:3] == (-(-hw[0] // stride), -(-hw[1] // stride))
    _close(got, want.reshape(-1, cout))


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("cout", [64, 72])
def test_depth_to_space_is_a_transposed_convolution_with_kernel_equal_to_stride(k, cout):
    B, Ho, Wo, cin = 2, 5, 7, 128
    x, w, b = _rand(4, B, Ho, Wo, cin), _rand(5, cin, cout, k, k), _rand(6, cout)
    got = rs.d2s(rs.product(x.reshape(-1, cin), rs.pack_convt(w)), b, B, Ho, Wo, k, cout)
    want = F.conv_transpose2d(_t(x).permute(0, 3, 1, 2), _t(w), _t(b), stride=k).permute(0, 2, 3, 1)
    _close(got, want)


@pytest.mark.parametrize("npad,npadv", [(40, 40), (40, 64), (264, 264)])
@pytest.mark.parametrize("table", [False, True])
def test_qkv_is_a_linear_layer_reshaped_to_heads(npad, npadv, table):
    B, heads, K = 3, 2, 128
    Fd = heads * 64
    x, w = _rand(7, B * npad, K), _rand(8, 3 * Fd, K)
    bias = _rand(9, B, 3 * Fd) if table else _rand(9, 3 * Fd)
    q, k, vt = rs.qkv(rs.product(x, w), bias, B, npad, npadv, heads, 0.125, bias_img_rows=npad)
    bt = _t(bias)[:, None] if table else _t(bias)
    y = (_t(x).reshape(B, npad, K) @ _t(w).T + bt).reshape(B, npad, 3, heads, 64).permute(2, 0, 3, 1, 4)  # [3, B, heads, npad, 64]
    _close(q, y[0] * 0.125)
    _close(k, y[1])
    _close(vt[..., :npad], y[2].transpose(-1, -2))
    assert np.isnan(vt[..., npad:]).all() and not np.isnan(vt[..., :npad]).any()


@pytest.mark.parametrize("cin", [64, 128])
@pytest.mark.parametrize("sigmoid", [False, True])
def test_head_is_conv_relu_pointwise_conv_and_the_final_activation(cin, sigmoid):
    B, H, W = 2, 9, 11
    x, w, b, hw_, hb = _rand(10, B, H, W, cin), _rand(11, 32, cin, 3, 3) / 8, _rand(12, 32), _rand(13, 32), 0.25
    got = rs.head(rs.product(rs.conv3_rows(x, 1), rs.pack_conv3(w)), b, hw_, hb, sigmoid)
    y = F.relu(F.conv2d(_t(x).permute(0, 3, 1, 2), _t(w), _t(b), padding=1))
    y = F.conv2d(y, _t(hw_).reshape(1, 32, 1, 1), torch.tensor([hb], dtype=torch.float64))
    y = torch.sigmoid(y) if sigmoid else F.relu(y)
    _close(got, y.reshape(-1))


def test_token_rows_are_the_slice_without_the_cls_and_pad_rows():
    B, tok_np, tok_stride, K, N = 3, 25, 32, 128, 64
    src, w, b = _rand(14, B * tok_stride, K), _rand(15, N, K), _rand(16, N)
    src3 = src.reshape(B, tok_stride, K).copy()
    got = rs.generic(rs.product(rs.token_rows(src, B, tok_np, tok_stride), w), b)
    src3[:, 0] = 1e30
    src3[:, 1 + tok_np:] = -1e30  # what must not be read cannot matter
    assert np.array_equal(rs.token_rows(src3.reshape(-1, K), B, tok_np, tok_stride), rs.token_rows(src, B, tok_np, tok_stride))
    want = F.linear(_t(src.reshape(B, tok_stride, K)[:, 1:1 + tok_np]), _t(w), _t(b))
    _close(got, want.reshape(-1, N))


@pytest.mark.parametrize("K", [192, 640])
@pytest.mark.parametrize("with_pos", [True, False])
def test_patch_is_the_linear_layer_plus_position_written_behind_the_cls_row(K, with_pos):
    B, tok_np, npad, N = 3, 25, 32, 128
    x, w, b, pos = _rand(17, B * tok_np, K), _rand(18, N, K), _rand(19, N), _rand(20, tok_np, N)
    got = rs.patch(rs.product(x, w), b, pos if with_pos else None, B, tok_np, npad).reshape(B, npad, N)
    want = F.linear(_t(x).reshape(B, tok_np, K), _t(w), _t(b))
    if with_pos:
        want = want + _t(pos)
    _close(got[:, 1:1 + tok_np], want)
    assert np.isnan(got[:, 0]).all() and np.isnan(got[:, 1 + tok_np:]).all()


def test_generic_epilogue_order_bias_table_and_k_ranges():
    M, N, K = 120, 64, 256
    a, w, table, gamma, resid = _rand(21, M, K), _rand(22, N, K), _rand(23, 3, N), _rand(24, N), _rand(25, M, N)
    acc = _t(a) @ _t(w).T
    want = F.relu(acc + _t(table).repeat_interleave(40, 0)) * _t(gamma) + _t(resid)
    _close(rs.generic(rs.product(a, w), table, 40, "relu", gamma, resid), want)
    for ks in (2, 4):
        planes = rs.ksplit_planes(a, w, ks)
        assert len(planes) == ks
        _close(sum(planes), acc)
        _close(planes[1], _t(a[:, K // ks:2 * K // ks]) @ _t(w[:, K // ks:2 * K // ks]).T)


def test_pass_terms_are_the_products_the_parameter_block_lists():
    M, N, K = 130, 128, 256
    ah, al, wh, wl = _rand(26, M, K), _rand(27, M, K) / 256, _rand(28, N, K), _rand(29, N, K) / 256
    _close(rs.pass_terms(ah, al, wh, wl, 1), _t(ah) @ _t(wh).T)
    _close(rs.pass_terms(ah, al, wh, wl, 2), (_t(ah) + _t(al)) @ _t(wh).T)
    _close(rs.pass_terms(ah, al, wh, wl, 3), (_t(ah) + _t(al)) @ (_t(wh) + _t(wl)).T - _t(al) @ _t(wl).T)
