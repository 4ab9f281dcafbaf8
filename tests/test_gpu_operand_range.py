"""The split-product forms across the activation range: fp8 cross terms (MDPT_PASSES_2F8 / _3F8, csrc/f8_cross.h), fp16-plane forms (per-class
2 / 3 passes, MDPT_PREC_FP16X3) and the bf16 forms, with every decoder activation scaled by 2^k. Run with `pytest -m gpu` on an MI355X.

Setup: the fp8-eligible Depth-Anything toy of test_gpu_f8_cross.py (F8_TOY) with EVERY decoder bias set to zero (reassembly, fusion, head).
The decoder is then positively homogeneous - convolutions without bias, ReLU, bilinear upsampling - so f(2^k x) = 2^k f(x) exactly in real
arithmetic, and in fp64 too (test_zero_bias_decoder_oracle_is_exactly_homogeneous). A form whose error grows with k has a range limit.

Scales: k in {-8, -4, 0, 4, 8, 10, 11, ..., k_max}, k_max the largest k with 2^k times the largest magnitude any decoder operand takes at k = 0
(measured on the oracle's intermediates) <= 32768 = OPERAND_MAX: the fp16 hi planes (65504) and the a8 plane (e5m2, 57344) stay unsaturated.

The lower end (OPERAND_MIN, include/mdpt.h). An fp16-plane split represents A as A_hi + A_lo with A_lo = fp16(A - A_hi). While A_lo is a normal
fp16 value the pair carries ~22 significant bits; fp16's subnormal quantum is 2^-24, so A_lo is rounded to an ABSOLUTE 2^-25 once |A_lo| < 2^-14,
i.e. once |A| < 2^-3 (|A_lo| <= 2^-12 |A|). The max-norm error of a contraction is set by its largest operands, so what matters is the largest
|A| of a tensor, M - but the typical element sits a few binades below M, so the floor shows before M itself reaches 2^-3. Measured (fp16x3,
reassembly / fusion / head, both launch shapes): the error is within 1.25x of its value at M ~ 4 down to M = 2^-2, 1.6 ... 2.8x at 2^-4,
~100x at 2^-10: OPERAND_MIN = 2^-2. The fp8 forms carry ~2^-15 relative error, so an absolute floor matters ~5 binades later: the fp8 residue
plane e5m2((A - A_hi) 2^11) is normal down to residues of 2^-25 (elements of 2^-13), and reassembly / fusion / the 2-term head stay within
1.2x down to M = 2^-9; the 3-term head, whose own error is smallest (2e-5), feeds a head tail on fp16 planes and shows that tail's 2^-25 floor
from M = 2^-6 (1.3x; 1.1x at 2^-5): OPERAND_MIN_F8 = 2^-5. The tests assert exactly [OPERAND_MIN(_F8), OPERAND_MAX], the ranges mdpt.h documents,
including the scale at each lower edge.

A. fp8 cross terms carry what fp16 cross terms carry at every scale: rel(y_f8, y_f16) <= 0.25 rel(y_1pass, y_f16), y_f16 the fp16-plane form with
   the same term count (the criterion of test_gpu_f8_cross.py). Before the residue shift was 11 (it was 16) the residue of |A| >= 2048
   saturated e5m2: this failed from k = 10 on (B from k = 8), where the largest operand passes 4096.
B. Flat error: rel(y_k, oracle_k) <= 1.3 rel(y_0, oracle_0) + 1e-6 for the fp16-plane and the fp8 forms over the documented range.
C. bf16 / bf16x3: every rounding commutes with x 2^k (bf16 has fp32's exponent range), so y(2^k x) == 2^k y(x) bit for bit.
   Exception, kept as a strict xfail: the fused bf16 head tail (test_bf16_fused_head_tail_is_exactly_scale_equivariant).
D. The whole DA-V2 toy in the default mixed mode (compensation on, batch split) with the reassembly input projections scaled by 2^k.
E. A BEiT toy whose stage taps (raw residual stream, no out-norm) carry massive-activation channels in the 2048 ... 8192 band.
"""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as TF

from tests.helpers import rel_err, seeded_input
from tests.test_gpu_f8_cross import F8_TOY, _oracle, _toy

pytestmark = pytest.mark.gpu

OPERAND_MAX = 32768.0       # include/mdpt.h: largest |activation| of a decoder operand the fp16 / fp8 split forms are specified for
OPERAND_MIN = 2.0 ** -2     # include/mdpt.h: the smallest largest-|activation| of an operand tensor down to which the fp16-plane forms hold
OPERAND_MIN_F8 = 2.0 ** -5  # include/mdpt.h: the same for the fp8 forms (MDPT_PASSES_2F8 / _3F8, the decoder of MDPT_PREC_MIXED)
REL_TOL_MIXED_TOY = 1.5e-3  # the mixed mode on toy configurations (test_gpu_precision_modes.py, smoke()): the encoder's single fp16 pass dominates
SHAPES = [(2, 56), (32, 112)]  # lockstep GEMM tiles; 8-phase GEMM + halo-staged conv + the two-stream split (images 0 and 31 checked)
BF16_KS = (-20, -7, 3, 17, 30)
_MODELS = {}


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from muggled_dpt_amd import native
    native.load()


def _zero_bias(osd):
    return {k: (torch.zeros_like(v) if k.startswith("depth_head.") and k.endswith(".bias") else v) for k, v in osd.items()}


def _weights64(osd):
    from muggled_dpt_amd.state_dict_conversion import convert_state_dict_keys, flatten_components, get_model_config_from_state_dict
    cfg = get_model_config_from_state_dict(osd)
    w = flatten_components(convert_state_dict_keys(cfg, osd))
    return cfg, {k: (v.double() if v.is_floating_point() else v) for k, v in w.items()}


def _model(osd, key, precision="fp16", passes=None, compensation=False):
    """A DA-V2 model of `osd`, cached under `key`; compensation None = the mode's default"""
    from muggled_dpt_amd import make_depthanythingv2_dpt_from_original_state_dict
    if key not in _MODELS:
        _, m = make_depthanythingv2_dpt_from_original_state_dict(osd)
        m = m.to("cuda", torch.float32)
        m.set_precision(precision)
        if compensation is not None:
            m.set_weight_rounding_compensation(compensation)
        if passes:
            m.set_class_passes(passes)
        _MODELS[key] = m
    return _MODELS[key]


class _Peak:
    """torch.nn.functional for the oracle, recording the largest magnitude any contraction / activation operand or result takes"""
    OPS = ("conv2d", "conv_transpose2d", "linear", "relu", "gelu", "interpolate")

    def __init__(self):
        self.peak = 0.0

    def __getattr__(self, name):
        fn = getattr(TF, name)
        if name not in self.OPS:
            return fn

        def rec(x, *a, **kw):
            y = fn(x, *a, **kw)
            self.peak = max(self.peak, float(x.abs().max()), float(y.abs().max()))
            return y
        return rec


def _oracle_with_peak(fn, *args):
    orc = _oracle()
    saved, p = orc.F, _Peak()
    orc.F = p
    try:
        with torch.inference_mode():
            y = fn(*args)
    finally:
        orc.F = saved
    return y, p.peak


def _k_max(peak):
    return math.floor(math.log2(OPERAND_MAX / peak))


def _k_min(peak, operand_min):
    return math.ceil(math.log2(operand_min / peak))


def _scales(peak):
    """k = 0 first (the baseline of B), then the sweep with the lower edges of the documented ranges"""
    km = _k_max(peak)
    ks = {-8, -4, 4, 8, *range(10, km + 1), _k_min(peak, OPERAND_MIN), _k_min(peak, OPERAND_MIN_F8)}
    return [0] + sorted(k for k in ks if k <= km and k != 0)


def _in_range(peak, k, operand_min):
    return operand_min <= peak * 2.0 ** k <= OPERAND_MAX


# ---- the stage-level cases: inputs at k = 0, the fp64 oracle at k = 0 on the checked images, the operand peak, and the three class configurations
F8_ALL = {"fusion": 5, "fusion_in": 5, "fusion_proj": 5}


def _cases(batch, size):
    from muggled_dpt_amd import native
    orc = _oracle()
    osd = _zero_bias(_toy(0)[0])
    cfg, w = _weights64(osd)
    g = size // 14
    chk = [0, batch - 1] if batch > 1 else [0]
    f8, f16 = native.PASSES_3F8, 3
    cases = []
    gen = torch.Generator().manual_seed(13)
    toks = [torch.randn(batch, 1 + g * g, 128, generator=gen) for _ in range(4)]
    refs, peak = _oracle_with_peak(orc.reassemble, w, [t[chk].double() for t in toks], (g, g))
    cases.append(dict(name="reasm", inputs=toks, refs=refs, peak=peak, run=lambda m, xs: m.reassemble(*xs, (g, g)),
                      passes=({"reasm": f8}, {"reasm": f16}, None)))
    sizes = [4 * g, 2 * g, g, g // 2]
    gen = torch.Generator().manual_seed(5)
    reasm = [torch.randn(batch, 256, s, s, generator=gen) * 2.0 for s in sizes]
    prev = None
    for i in (3, 2, 1, 0):
        inputs = [reasm[i]] if prev is None else [reasm[i], prev]
        ref, peak = _oracle_with_peak(orc.fusion_block, w, i, reasm[i][chk].double(), None if prev is None else prev[chk].double())
        # (head = 3 in all three: with a single-pass head block 0 hands over a 16-bit map instead of the fp32 one)
        cases.append(dict(name=f"fusion.blocks[{i}]", inputs=inputs, refs=[ref], peak=peak, run=lambda m, xs, i=i: [m.fusion.blocks[i](*xs)],
                          passes=({**F8_ALL, "head": 3}, {"fusion": 3, "fusion_in": 3, "fusion_proj": 3, "head": 3}, {"head": 3})))
        prev = orc.fusion_block(w, i, reasm[i].double(), None if prev is None else prev.double()).float()  # exact previous map: no compounding
    fused = torch.randn(batch, 256, 8 * g, 8 * g, generator=torch.Generator().manual_seed(9)) * 1.5
    ref, peak = _oracle_with_peak(orc.head, w, cfg, fused[chk].double())
    for terms, f8v in ((2, native.PASSES_2F8), (3, native.PASSES_3F8)):
        cases.append(dict(name=f"head ({terms} terms)", inputs=[fused], refs=[ref], peak=peak, run=lambda m, xs: [m.head(*xs)],
                          passes=({"head": f8v, "head_tail": 3}, {"head": terms, "head_tail": 3}, {"head_tail": 3})))
    return osd, chk, cases


def _run(model, case, k, chk=None):
    """the case's outputs at scale k: images `chk` on the host, or every image on the device (chk None)"""
    xs = [(x * 2.0 ** k).cuda() for x in case["inputs"]]
    return [y if chk is None else y[chk].cpu() for y in case["run"](model, xs)]


@pytest.mark.parametrize("batch,size", SHAPES)
def test_split_forms_across_the_operand_range(batch, size):
    """A (fp8 cross terms vs fp16 cross terms at every scale) and B (flat error against the oracle over [OPERAND_MIN, OPERAND_MAX])."""
    osd, chk, cases = _cases(batch, size)
    rows, fails = [], []
    for case in cases:
        f8p, f16p, onep = case["passes"]
        tag = case["name"]
        m8 = _model(osd, ("f8", tag), passes=f8p)
        m16 = _model(osd, ("f16", tag), passes=f16p)
        m1 = _model(osd, ("1", tag), passes=onep)
        mx3 = _model(osd, ("fp16x3",), precision="fp16x3")
        base = {}
        for k in _scales(case["peak"]):
            outs = {f: _run(m, case, k, chk) for f, m in (("f8", m8), ("f16", m16), ("1", m1), ("fp16x3", mx3))}
            for j, ref in enumerate(case["refs"]):
                name = f"{tag}[{j}]" if len(case["refs"]) > 1 else tag
                ref_k = ref * 2.0 ** k
                e = {f: rel_err(o[j], ref_k) for f, o in outs.items()}
                a_num, a_den = rel_err(outs["f8"][j], outs["f16"][j]), rel_err(outs["1"][j], outs["f16"][j])
                rows.append(f"{name:22s} k={k:3d} peak={case['peak'] * 2.0 ** k:9.3g}  A: f8 vs f16 {a_num:.2e}  1-pass vs f16 {a_den:.2e}  "
                            f"B: f8 {e['f8']:.2e} f16 {e['f16']:.2e} fp16x3 {e['fp16x3']:.2e}")
                if not a_num <= 0.25 * a_den:
                    fails.append(f"A {name} k={k}: {a_num:.3e} > 0.25 x {a_den:.3e}")
                if k == 0:
                    base[name] = e
                else:
                    for f in ("f8", "f16", "fp16x3"):
                        if _in_range(case["peak"], k, OPERAND_MIN_F8 if f == "f8" else OPERAND_MIN) and not e[f] <= 1.3 * base[name][f] + 1e-6:
                            fails.append(f"B {name} {f} k={k}: {e[f]:.3e} > 1.3 x {base[name][f]:.3e} + 1e-6")
    print("\n" + "\n".join(rows))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("batch,size", SHAPES)
def test_bf16_forms_are_exactly_scale_equivariant(batch, size):
    """C. bf16 operands keep fp32's exponent range and every other rounding (fp32 accumulation, the fp32 bilinear upsample, ReLU) commutes with
    x 2^k: y(2^k x) == 2^k y(x) bit for bit. A difference is a constant that is not homogeneous (an epsilon, a clamp, a threshold) in a kernel."""
    osd, _, cases = _cases(batch, size)
    for precision in ("bf16", "bf16x3"):
        m = _model(osd, (precision,), precision=precision)
        for case in cases[:-1]:  # (the head has no class passes in these modes: one case)
            if precision == "bf16" and case["name"].startswith("head"):
                continue  # the fused head tail: test_bf16_fused_head_tail_is_exactly_scale_equivariant
            y0 = _run(m, case, 0)
            for k in BF16_KS:
                yk = _run(m, case, k)
                for j, (a, b) in enumerate(zip(yk, y0)):
                    assert torch.equal(a, b * 2.0 ** k), f"{precision} {case['name']}[{j}] k={k}: max |diff| {float((a - b * 2.0 ** k).abs().max()):.3e}"


@pytest.mark.xfail(strict=True, reason="head_tail_kernel reads the odd bf16 element of a pair in place (see the docstring)")
@pytest.mark.parametrize("batch,size", SHAPES)
def test_bf16_fused_head_tail_is_exactly_scale_equivariant(batch, size):
    """C for the head in bf16, a KNOWN FAILURE. The fused head tail (head.hip, head_tail_kernel) converts the odd bf16 element of a packed pair
    by using the dword in place: its low 16 bits are the neighbour's bf16 bits, a relative perturbation below 2^-16 that depends on the
    NEIGHBOUR's exponent - so it changes under x 2^k, flips bf16 roundings of the upsampled map, and the depth map moves by 0.6 ... 1.6e-3
    relative (the mode's own error against the oracle: 5e-3). Masking the low half makes it exact (measured: this test passes), but re-rounds
    the bf16 map: test_gpu_model_fuzz.py cfg9 then reads 1.751e-2 against its 1.639e-2 tolerance (1.590e-2 now). Strict: the day the
    kernel is fixed this reports XPASS and the exemption in test_bf16_forms_are_exactly_scale_equivariant goes."""
    osd, _, cases = _cases(batch, size)
    m = _model(osd, ("bf16",), precision="bf16")
    case = [c for c in cases if c["name"].startswith("head")][0]
    y0 = _run(m, case, 0)
    for k in BF16_KS:
        assert torch.equal(_run(m, case, k)[0], y0[0] * 2.0 ** k), k


def test_zero_bias_decoder_oracle_is_exactly_homogeneous():
    """The premise of this file, checked once in fp64: with zero decoder biases, the oracle at 2^k times the input (or the reassembly input
    projections times 2^k) is 2^k times the oracle, bit for bit."""
    orc = _oracle()
    osd = _zero_bias(_toy(0)[0])
    cfg, w = _weights64(osd)
    x = seeded_input((1, 3, 56, 56), 3).double()
    y0, st = orc.forward(w, cfg, x, return_stages=True)
    for k in (-8, 13):
        osd_k = _scaled_projections(osd, k)
        _, wk = _weights64(osd_k)
        assert torch.equal(orc.forward(wk, cfg, x), y0 * 2.0 ** k), k
        s = 2.0 ** k
        assert all(torch.equal(a, b * s) for a, b in zip(orc.reassemble(w, [t * s for t in st["stages"]], st["grid_hw"]),
                                                            orc.reassemble(w, st["stages"], st["grid_hw"])))
        assert torch.equal(orc.fusion(w, [r * s for r in st["reasm"]]), st["fused"] * s)
        assert torch.equal(orc.head(w, cfg, st["fused"] * s), y0 * s)


def _scaled_projections(osd, k):
    return {n: (v * 2.0 ** k if n.startswith("depth_head.projects.") and n.endswith(".weight") else v) for n, v in osd.items()}


@pytest.mark.parametrize("batch,size", SHAPES)
def test_default_mixed_mode_end_to_end_across_the_range(batch, size):
    """D. The whole DA-V2 toy in the default mixed mode (fp8 decoder classes, compensation on, batch split at 32) with the four reassembly input
    projections scaled by 2^k: every decoder activation and the depth map scale by 2^k, the error against the oracle must not grow."""
    orc = _oracle()
    osd = _zero_bias(_toy(0)[0])
    cfg, w = _weights64(osd)
    x = seeded_input((batch, 3, size, size), 21)
    chk = [0, batch - 1]
    ref0, st = orc.forward(w, cfg, x[chk].double(), return_stages=True)
    peak = 0.0
    for fn, args in ((orc.reassemble, (w, st["stages"], st["grid_hw"])), (orc.fusion, (w, st["reasm"])), (orc.head, (w, cfg, st["fused"]))):
        peak = max(peak, _oracle_with_peak(fn, *args)[1])
    errs = {}
    for k in [k for k in _scales(peak) if k >= 0]:
        m = _model(_scaled_projections(osd, k), ("mixed", k), precision="mixed", compensation=None)
        errs[k] = rel_err(m(x.cuda())[chk].cpu(), ref0 * 2.0 ** k)
        del _MODELS[("mixed", k)]
    print(f"\nmixed, batch {batch}, decoder operand peak {peak:.3g} at k = 0: " + ", ".join(f"k={k} {e:.3e}" for k, e in errs.items()))
    for k, e in errs.items():
        assert e <= REL_TOL_MIXED_TOY and e <= 1.3 * errs[0], f"k={k}: {e:.3e} (k = 0: {errs[0]:.3e})"


BEIT_F8_TOY = dict(features_per_token=128, num_heads=2, num_blocks=4, reassembly_features_list=[128, 128, 256, 256], base_patch_grid_hw=(4, 4),
                   fusion_channels=256, patch_size_px=16)


def test_beit_raw_taps_with_massive_activation_channels_keep_the_f8_reassembly_accurate():
    """E. BEiT's reassembly reads the raw residual stream (no out-norm). Two massive-activation channels (block 0's fc2 bias +6000 / -3000, its
    layer scale 1 there; synthetic.realistic_statistics has the same construction at +150 / -90) put every stage tap's largest values in the
    2048 ... 8192 band: the fp8 reassembly has to stay as accurate as three fp16-plane passes."""
    from muggled_dpt_amd import make_beit_dpt_from_midas_v31_state_dict, native
    from muggled_dpt_amd import state_dict_conversion_beit as conv
    from muggled_dpt_amd.state_dict_conversion import flatten_components
    from muggled_dpt_amd.synthetic import make_synthetic_beit_state_dict
    orc = _oracle()
    osd = make_synthetic_beit_state_dict(BEIT_F8_TOY, 0)
    f = BEIT_F8_TOY["features_per_token"]
    bias, gamma = osd["pretrained.model.blocks.0.mlp.fc2.bias"], osd["pretrained.model.blocks.0.gamma_2"]
    bias[7] += 6000.0
    bias[f // 2 + 9] -= 3000.0
    gamma[7] = gamma[f // 2 + 9] = 1.0
    cfg, _ = make_beit_dpt_from_midas_v31_state_dict(osd)
    w = flatten_components(conv.convert_state_dict_keys(cfg, osd))
    x = seeded_input((2, 3, 128, 128), 23)
    ref, st = orc.forward(w, cfg, x, return_stages=True)
    tap_peaks = [float(t.abs().max()) for t in st["stages"]]
    print(f"\nBEiT stage tap peaks: {tap_peaks}")
    assert all(2048.0 <= p <= 8192.0 for p in tap_peaks), tap_peaks
    errs = {}
    for reasm in (native.PASSES_3F8, 3):
        _, m = make_beit_dpt_from_midas_v31_state_dict(osd)
        m = m.to("cuda", torch.float32)
        m.set_precision("mixed")
        m.set_class_passes({"reasm": reasm})
        y = m(x.cuda())
        if reasm == native.PASSES_3F8:
            got = ctypes.c_int(-1)
            lib = native.load()
            native.check(lib, lib.mdpt_get_class_f8(m._get_engine().handle, native.OP_CLASSES.index("reasm"), ctypes.byref(got)))
            assert got.value == 1, "the BEiT toy must run the fp8 form of the reassembly"
        errs[reasm] = rel_err(y.cpu(), ref)
    print(f"BEiT mixed: reasm fp8 cross terms {errs[native.PASSES_3F8]:.3e}, fp16 planes {errs[3]:.3e}")
    assert errs[native.PASSES_3F8] <= 1.25 * errs[3] + 2e-6
