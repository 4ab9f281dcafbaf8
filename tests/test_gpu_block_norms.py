"""DPTModel.block_norms / ImageEncoder.block_norms (mdpt_encoder_block_norms): the per-token L2 norms of every transformer block's output, what
the reference's experiments/block_norm_visualization.py:133-147 keeps of the tensors it captures with forward hooks, computed on the fp32
residual stream inside the encoder pass without exporting a block tensor. The yardstick is the hook path of the same build
(mdpt_encoder_probe_blocks, tied to the oracle by tests/test_gpu_block_hooks.py), and the oracle's own per-block capture. `pytest -m gpu`.

Bounds (set by the issue, not by what the code gives):
  fp32 model   |norm - ||hook tokens||_2 (fp64)| <= 2e-6 * norm per element. The kernel adds at most F / 64 = 24 terms serially per lane at
               F = 1536 and 6 more in the wave reduction: a relative error of the sum of at most 30 * 2^-24, halved by the sqrt, plus one rounding
               for the sqrt and one per square.
  bf16 model   the hook hands out the tokens rounded to bf16 (each within 2^-9 relative): <= 2^-8 * norm.
  oracle       e_cap <= e_hook + 2e-6 with e = rel_err(., ||oracle block output||): the capture is no further from the oracle than the hook path."""
import ctypes
import json

import pytest
import torch

from tests.helpers import rel_err, seeded_input, synthetic_model

pytestmark = pytest.mark.gpu

FP32_BOUND = 2e-6
BF16_BOUND = 2.0 ** -8
CASES = [("v2", (56, 84)), ("beit", (64, 96)), ("swinv2", (64, 96)), ("v1", (56, 84))]
DTYPES = [torch.float32, torch.bfloat16]


def _oracle():
    from oracle import dpt_oracle
    return dpt_oracle


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from muggled_dpt_amd import native
    native.load()


def _build(family, dtype):
    """v2 `tiny`, `beit_tiny`, `swin2_tiny` and the 8-block V1 model, as tests/test_gpu_block_hooks.py builds them -> (model, cfg, oracle weights)"""
    import muggled_dpt_amd as mda
    from muggled_dpt_amd.state_dict_conversion import flatten_components
    if family == "beit":
        from muggled_dpt_amd import state_dict_conversion_beit as conv
        from muggled_dpt_amd.synthetic import make_synthetic_beit_state_dict
        osd = make_synthetic_beit_state_dict("beit_tiny", 3)
        cfg, model = mda.make_beit_dpt_from_midas_v31_state_dict(osd)
        w = flatten_components(conv.convert_state_dict_keys(cfg, osd))
    elif family == "swinv2":
        from muggled_dpt_amd import state_dict_conversion_swinv2 as conv
        from muggled_dpt_amd.synthetic import make_synthetic_swinv2_state_dict
        osd = make_synthetic_swinv2_state_dict("swin2_tiny", 5)
        cfg, model = mda.make_swinv2_dpt_from_midas_v31_state_dict(osd)
        w = flatten_components(conv.convert_state_dict_keys(cfg, osd))
    elif family == "v1":
        from muggled_dpt_amd.synthetic import STANDARD_CONFIGS, make_synthetic_original_state_dict
        osd = make_synthetic_original_state_dict(dict(STANDARD_CONFIGS["tiny"], num_blocks=8), 3)
        cfg, model = mda.make_depthanythingv1_dpt_from_original_state_dict(osd)
        cfg = {**cfg, "num_blocks": 8}
        w = {f"{comp}.{k}": v.detach().float().cpu() for comp in ("patch_embed", "imgencoder", "reassemble", "fusion", "head")
             for k, v in getattr(model, comp).state_dict().items()}
    else:
        osd, cfg, w = synthetic_model("tiny", 0)
        cfg, model = mda.make_depthanythingv2_dpt_from_original_state_dict(osd)
    return model.to("cuda", dtype), cfg, w


def _blocks(model, cfg, family):
    if family == "swinv2":
        return [model.imgencoder.stages[s].blocks[l] for s, nl in enumerate(cfg["layers_per_stage"]) for l in range(int(nl))]
    if family == "v1":
        return [model.imgencoder.blocks[i] for i in range(cfg["num_blocks"])]
    bps = cfg["num_blocks"] // 4
    return [model.imgencoder.stages[i // bps].blocks[i % bps] for i in range(cfg["num_blocks"])]


def _grids(cfg, family, grid):
    if family == "swinv2":
        return [(grid[0] >> s, grid[1] >> s) for s, nl in enumerate(cfg["layers_per_stage"]) for _ in range(int(nl))]
    return [tuple(grid)] * cfg["num_blocks"]


def _features(cfg, family):
    if family == "swinv2":
        return [int(cfg["features_per_stage"][s]) for s, nl in enumerate(cfg["layers_per_stage"]) for _ in range(int(nl))]
    return [int(cfg["features_per_token"])] * cfg["num_blocks"]


def _hook_tokens(model, cfg, family, x):
    """every block's output tokens through the hook path (patch_embed -> imgencoder with a forward hook on every block), patch tokens only"""
    blocks = _blocks(model, cfg, family)
    got = {}
    handles = [blk.register_forward_hook(lambda mod, args, out, i=i: got.__setitem__(i, out)) for i, blk in enumerate(blocks)]
    try:
        with torch.inference_mode():
            tokens, hw = model.patch_embed(x)
            model.imgencoder(tokens, hw)
    finally:
        for h in handles:
            h.remove()
    assert sorted(got) == list(range(len(blocks)))
    skip = 0 if family == "swinv2" else 1  # the cls token
    return [got[i][:, skip:] for i in range(len(blocks))]


def _oracle_blocks(w, cfg, family, x):
    orc = _oracle()
    tokens, grid = orc.patch_embed(w, x)
    ref = []
    enc = {"beit": orc.beit_image_encoder, "swinv2": orc.swin_image_encoder}.get(family, orc.image_encoder)
    enc(w, cfg, tokens, grid, block_outputs=ref)
    skip = 0 if family == "swinv2" else 1
    return [r[:, skip:] for r in ref]


def _norm_err(norms, hooked, grids):
    """max over every element of every block of |norm - ||hook tokens||_2| / ||hook tokens||_2, the hook norm in fp64"""
    worst = 0.0
    for n, t, (h, w) in zip(norms, hooked, grids):
        ref = t.double().norm(dim=-1).reshape(t.shape[0], h, w)
        assert bool((ref > 0).all())
        worst = max(worst, float(((n.double() - ref).abs() / ref).max()))
    return worst


def _profile_names(fn):
    """kernel names the library launched while fn() ran (mdpt_profile_enable / report)"""
    from muggled_dpt_amd import native
    lib = native.load()
    native.check(lib, lib.mdpt_profile_enable(1))
    try:
        try:
            fn()
        finally:
            torch.cuda.synchronize()
            buf = ctypes.create_string_buffer(1 << 20)
            native.check(lib, lib.mdpt_profile_report(buf, len(buf)))
    finally:
        native.check(lib, lib.mdpt_profile_enable(0))
    return {k["name"]: k for k in json.loads(buf.value.decode())["kernels"]}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family,hw", CASES)
def test_block_norms_match_the_hook_path(family, hw, dtype):
    model, cfg, w = _build(family, dtype)
    x = seeded_input((2, 3, *hw), seed=13).to("cuda", dtype)
    seen = []
    listener = _blocks(model, cfg, family)[1].register_forward_hook(lambda mod, args, out: seen.append(out))
    norms, grid = model.block_norms(x)
    listener.remove()
    assert not seen, "a forward hook fired during block_norms"
    grids = _grids(cfg, family, grid)
    # one fp32 [2, h_l, w_l] map per block; SwinV2 maps shrink by stage; views into one allocation
    assert len(norms) == len(_blocks(model, cfg, family)) == len(grids)
    for n, (h, wd) in zip(norms, grids):
        assert n.dtype == torch.float32 and n.is_cuda and tuple(n.shape) == (2, h, wd)
    assert len({n.untyped_storage().data_ptr() for n in norms}) == 1
    if family == "swinv2":
        assert grids[0] == (16, 24) and grids[-1] == (2, 3) and len({g for g in grids}) == 4
    hooked = _hook_tokens(model, cfg, family, x)
    err = _norm_err(norms, hooked, grids)
    bound = FP32_BOUND if dtype == torch.float32 else BF16_BOUND
    print(f"{family} {dtype}: max |norm - hook norm| / norm = {err:.3e} (bound {bound:.3e})")
    assert err <= bound, f"{family} {dtype}: {err:.3e} > {bound:.3e}"


@pytest.mark.parametrize("family,hw", CASES)
def test_block_norms_against_the_oracle_fp32(family, hw):
    model, cfg, w = _build(family, torch.float32)
    x = seeded_input((2, 3, *hw), seed=13)
    norms, grid = model.block_norms(x.cuda())
    grids = _grids(cfg, family, grid)
    hooked = _hook_tokens(model, cfg, family, x.cuda())
    ref = _oracle_blocks(w, cfg, family, x)
    assert len(ref) == len(norms)
    e_hook = e_cap = 0.0
    for n, t, r, (h, wd) in zip(norms, hooked, ref, grids):
        want = r.double().norm(dim=-1).reshape(2, h, wd)
        e_hook = max(e_hook, rel_err(t.double().cpu().norm(dim=-1).reshape(2, h, wd), want))
        e_cap = max(e_cap, rel_err(n.cpu(), want))
    print(f"{family}: rel_err to the oracle's block norms: hook path e_hook = {e_hook:.3e}, block_norms e_cap = {e_cap:.3e}")
    assert e_cap <= e_hook + 2e-6, f"{family}: e_cap {e_cap:.3e} > e_hook {e_hook:.3e} + 2e-6"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family,hw", CASES)
def test_channel_planes_are_the_hook_tokens_channel(family, hw, dtype):
    model, cfg, w = _build(family, dtype)
    x = seeded_input((2, 3, *hw), seed=21).to("cuda", dtype)
    feats = _features(cfg, family)
    chans = [(7 * l + 3) % f if l else f - 1 for l, f in enumerate(feats)]  # the last channel once, then a different one per block
    norms, planes, grid = model.block_norms(x, channels=chans)
    grids = _grids(cfg, family, grid)
    hooked = _hook_tokens(model, cfg, family, x)
    norms_only, _ = model.block_norms(x)
    for l, (p, t, (h, wd)) in enumerate(zip(planes, hooked, grids)):
        assert p.dtype == torch.float32 and tuple(p.shape) == (2, h, wd)
        want = t[:, :, chans[l]].reshape(2, h, wd)
        assert torch.equal(p if dtype == torch.float32 else p.to(dtype), want), f"block {l} channel {chans[l]}"
        assert torch.equal(norms[l], norms_only[l])  # asking for a channel does not change the norms
    # one int for every block
    _, planes5, _ = model.block_norms(x, channels=5)
    for l, (p, t, (h, wd)) in enumerate(zip(planes5, hooked, grids)):
        assert torch.equal(p if dtype == torch.float32 else p.to(dtype), t[:, :, 5].reshape(2, h, wd)), f"block {l} channel 5"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family,hw", CASES)
def test_a_rows_norms_do_not_depend_on_its_batch(family, hw, dtype):
    model, cfg, w = _build(family, dtype)
    x = seeded_input((2, 3, *hw), seed=5).to("cuda", dtype)
    both, planes, _ = model.block_norms(x, channels=1)
    for b in range(2):
        one, plane1, _ = model.block_norms(x[b:b + 1], channels=1)
        for l, (n2, n1) in enumerate(zip(both, one)):
            assert torch.equal(n2[b:b + 1], n1), f"image {b} block {l}"
            assert torch.equal(planes[l][b:b + 1], plane1[l]), f"image {b} block {l} (channel)"


@pytest.mark.parametrize("family,hw", CASES)
def test_block_norms_leave_the_forward_alone(family, hw):
    model, cfg, w = _build(family, torch.float32)
    x = seeded_input((2, 3, *hw), seed=8).cuda()
    y_before = model(x)
    with torch.inference_mode():
        tokens, grid = model.patch_embed(x)
        want_taps = model.imgencoder(tokens, grid)
        fired = []
        listener = _blocks(model, cfg, family)[0].register_forward_hook(lambda mod, args, out: fired.append(out))
        names = _profile_names(lambda: fired.append(model.imgencoder.block_norms(tokens, grid)))
        listener.remove()
    taps, norms = fired.pop()
    assert not fired, "a forward hook fired during block_norms"
    assert names["row_norm_kernel"]["launches"] == len(norms)  # one launch per block, where the hook path exports that block's tokens
    assert len(taps) == 4
    for t, wt in zip(taps, want_taps):
        assert t.dtype == wt.dtype and torch.equal(t, wt)
    assert torch.equal(model(x), y_before)


@pytest.mark.parametrize("family,hw", CASES)
def test_latency_mode_leaves_no_partial_sums_out_of_the_norms(family, hw):
    """Latency mode splits K of proj / fc2 at small batches and lets the next LayerNorm add the partial sums: a block whose norms are wanted
    must be complete when the row-norm kernel reads it, like a block whose raw output is exported."""
    from muggled_dpt_amd import native
    model, cfg, w = _build(family, torch.float32)
    model.set_latency_mode(True)
    x = seeded_input((1, 3, *hw), seed=13).cuda()
    y = model(x)  # engine exists now
    eng = model._get_engine()
    native.check(eng.lib, eng.lib.mdpt_debug_set_ksplit_min(eng.handle, 2, 1 << 30))  # the toy models' fc2 has 4 K tiles: split it
    names = _profile_names(lambda: model(x))
    if family != "swinv2":  # (SwinV2 decides its K split by K alone, in every mode)
        assert "layernorm_addp_kernel" in names, sorted(names)  # the split is live in the plain forward of this mode
    norms, grid = model.block_norms(x)
    grids = _grids(cfg, family, grid)
    hooked = _hook_tokens(model, cfg, family, x)
    err = _norm_err(norms, hooked, grids)
    print(f"{family} latency mode: max |norm - hook norm| / norm = {err:.3e} (bound {FP32_BOUND:.3e})")
    assert err <= FP32_BOUND
    del y


def test_a_bad_channel_index_raises_and_launches_nothing():
    from muggled_dpt_amd import native
    model, cfg, w = _build("swinv2", torch.float32)
    x = seeded_input((1, 3, 64, 96), seed=2).cuda()
    with torch.inference_mode():
        tokens, (gh, gw) = model.patch_embed(x)
    eng = model._get_engine()
    torch.cuda.synchronize()

    def python_level():
        with pytest.raises(ValueError, match="outside"):
            model.imgencoder.block_norms(tokens, (gh, gw), channels=64)  # stage 0 has 64 features
        with pytest.raises(ValueError, match="blocks but"):
            model.imgencoder.block_norms(tokens, (gh, gw), channels=[0, 1])
    assert _profile_names(python_level) == {}

    # the C entry itself: index 128 is fine for stages 1-3 but not for the two blocks of stage 0
    grids = _grids(cfg, "swinv2", (gh, gw))
    outs = [torch.empty((1, (gh >> s) * (gw >> s), eng.stage_features[s]), device="cuda") for s in range(4)]
    norms = [torch.full((1, h, wd), -1.0, device="cuda") for h, wd in grids]
    planes = [torch.full((1, h, wd), -1.0, device="cuda") for h, wd in grids]
    narr = (ctypes.c_void_p * len(norms))(*[t.data_ptr() for t in norms])
    parr = (ctypes.c_void_p * len(planes))(*[t.data_ptr() for t in planes])
    for bad in ([100] * 10, [0] * 9 + [-1], [0, 0, 0, 128, 0, 0, 0, 0, 0, 0]):
        idx = (ctypes.c_int32 * 10)(*bad)

        def c_level():
            with pytest.raises(native.MdptError) as e:
                eng.call("mdpt_encoder_block_norms", tokens.float().contiguous(), 1, gh, gw, eng.ptr_array(outs), narr, idx, parr,
                         size_hw=(gh * eng.P, gw * eng.P), batch=1)
            assert e.value.code == -1 and "channel index" in str(e.value)
        assert _profile_names(c_level) == {}
    torch.cuda.synchronize()
    assert all(bool((t == -1.0).all()) for t in norms + planes)
    # ... and the same call with legal indices fills everything
    idx = (ctypes.c_int32 * 10)(*[63, 63, 127, 127, 255, 255, 255, 255, 511, 511])
    eng.call("mdpt_encoder_block_norms", tokens.float().contiguous(), 1, gh, gw, eng.ptr_array(outs), narr, idx, parr, size_hw=(gh * eng.P, gw * eng.P), batch=1)
    torch.cuda.synchronize()
    assert all(bool((t > 0).all()) for t in norms) and all(bool((t != -1.0).all()) for t in planes)
