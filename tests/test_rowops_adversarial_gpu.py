"""ln_kernel (plain and EMBED form), the fused and the stand-alone MLP activation on planted inputs with per-element bounds
(tests/_rowop_cases.py: the cases, the float64 references, the bounds and where each comes from).  Run with ``-m gpu`` on an MI355X.

LayerNorm: a hook that returns the planted [B, T, d] tensor puts it in front of one LayerNorm of a two-layer model -- 15 rows (3 images
of 5 tokens), so the last 4-row workgroup holds 3:

    entry point (hook)                          LayerNorm      d_model (8-element chunks; register chunk c of lane L is chunk L + 64 c)
    blocks.0.hook_resid_pre                     blocks.0.ln1   520  (65: register chunk 1 holds lane 0 only)
    blocks.1.hook_resid_pre (mid-model)         blocks.1.ln1   1032 (129: register chunk 2 holds lane 0 only)
    blocks.0.hook_resid_mid                     blocks.0.ln2   8 (1 chunk), 136 (17: register chunk 0 partly filled)
    blocks.1.hook_resid_post                    ln_final       1544 (193: register chunk 3 holds lane 0 only), 2048 (256: all full)

hook_scale and hook_normalized are fp32 in both dtypes; the bf16 LayerNorm output is exposed by hook_ln_final (and by hook_ln_pre in
the EMBED form) only -- ln1's and ln2's feed the next GEMM from the workspace -- and where it is, it must be the fp32 tap rounded.

The EMBED form (cls / patch + pos, rounded, then ln_pre) takes no hook: W_pos, the cls token and the conv bias are planted rows and the
conv weight is 0, so row(b, t) = round(e + pos[t]) is known exactly.

The activation: every finite bf16 value (and 65 536 fp32 values that are no bf16 values) through the ACT epilogue of pv_gemm_epilogue
in one 256^3 launch (A the identity, B the values, bias 0: out0 must be the values, out1 their activation), under gemm_tile 0, 4, 5;
and all 65 536 bit patterns, the non-finite ones included, through pv_launch_act behind a hook on mlp.hook_pre, whose output must have
the bits of the fused epilogue's.
"""
import functools

import pytest
import torch

from vit_prisma_amd import HookedViT, HookedViTConfig, _native

import _rowop_cases as RC

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
B, T = 3, 5                                              # image 8, patch 4, cls token
ENTRY = {8: "ln2", 136: "ln2", 520: "ln1", 1032: "ln1_mid", 1544: "ln_final", 2048: "ln_final"}
SITE = {  # entry -> (hooked point, prefix of the LayerNorm's points, the point that exposes its output in the storage dtype)
    "ln1": ("blocks.0.hook_resid_pre", "blocks.0.ln1.", None),
    "ln1_mid": ("blocks.1.hook_resid_pre", "blocks.1.ln1.", None),
    "ln2": ("blocks.0.hook_resid_mid", "blocks.0.ln2.", None),
    "ln_final": ("blocks.1.hook_resid_post", "ln_final.", "hook_ln_final"),
}


def _name(dtype):
    return "bf16" if dtype == BF16 else "fp32"


def _same(got, want):
    """equal values, NaN where NaN (the sign of a zero is not compared)"""
    got, want = got.float().cpu(), want.float().cpu()
    return got.shape == want.shape and bool(((got == want) | (torch.isnan(got) & torch.isnan(want))).all())


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def _vit(dtype, d_model, n_layers, d_mlp, image_size=8, activation="gelu", layer_norm_pre=True, n_heads=1):
    cfg = dict(n_layers=n_layers, d_model=d_model, n_heads=n_heads, d_head=32, d_mlp=d_mlp, patch_size=4, image_size=image_size,
               n_channels=3, n_classes=16, eps=RC.LN_EPS, layer_norm_pre=layer_norm_pre, normalize_output=True,
               return_type="class_logits", activation_name=activation, use_cls_token=True, normalization_type="LN",
               classification_type="cls")
    torch.manual_seed(d_model + n_layers)
    return HookedViT(HookedViTConfig(**cfg, dtype=dtype, device="cuda")).to(dtype).cuda().eval().use_native(True)


@functools.lru_cache(maxsize=None)
def _ln_model(dtype, d):
    model = _vit(dtype, d, 2, 64)
    assert model.n_tokens == T
    x = torch.randn(B, 3, 8, 8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(d)).to(dtype)
    return model, x


def _layer_norms(model):
    mods = [model.ln_final] + ([model.ln_pre] if model.cfg.layer_norm_pre else [])
    for blk in model.blocks:
        mods += [blk.ln1, blk.ln2]
    return mods


def _plant_ln_weights(model, w, b):
    with torch.no_grad():
        for m in _layer_norms(model):
            m.w.copy_(w.to(m.w.dtype))
            m.b.copy_(b.to(m.b.dtype))
    model.invalidate_native_weights()


def _run(model, x, hooks=(), names_filter=None):
    with torch.no_grad():
        _, cache = model.run_with_cache(x, fwd_hooks=list(hooks), names_filter=names_filter)
    assert model.last_run_native, model.native_fallback_reason
    return {k: v.clone() for k, v in cache.items()}


# ------------------------------------------------------------------------------------------------------------- LN1, LN2, ln_final
@pytest.mark.parametrize("d", sorted(ENTRY))
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_name)
def test_layer_norm_on_planted_rows(dtype, d):
    bf16 = dtype == BF16
    model, images = _ln_model(dtype, d)
    point, pre, out_point = SITE[ENTRY[d]]
    worst, beside = {}, {}
    for planted in (True, False):
        w, b = RC.ln_weights(d, planted)
        _plant_ln_weights(model, w, b)
        for name in RC.LN_CASES:
            x = RC.ln_rows(name, B * T, d)
            plant = x.view(B, T, d).to(dtype).cuda()
            hooks = [(point, lambda t, hook=None, r=plant: r)]
            cache = _run(model, images, hooks)                                                         # every tap
            assert _same(cache[point], x.view(B, T, d)), (name, "the LayerNorm was not handed the planted rows")
            scale, norm = cache[pre + "hook_scale"], cache[pre + "hook_normalized"]
            assert scale.dtype == F32 and scale.shape == (B, T, 1) and norm.shape == (B, T, d)
            assert norm.dtype == F32                                                                    # (the fp32 tap in bf16 mode)
            y16 = None
            if out_point is not None:
                out = cache[out_point]
                assert out.dtype == dtype and out.shape == (B, T, d)
                if bf16:
                    y16 = out
                    assert _same_bits(out, norm.to(BF16)), (name, "the bf16 output is not the fp32 tap rounded")
                else:
                    assert _same_bits(out, norm)
            r = RC.check_ln(x, w, b, scale=scale.cpu().view(-1), y32=norm.cpu().view(-1, d), y16=None if y16 is None else y16.cpu().view(-1, d))
            t = RC.ln_torch_ratios(x, w, b, bf16=y16 is not None)
            line = RC.report(f"{_name(dtype)} d={d} {ENTRY[d]} {'planted' if planted else 'default'} w, b  {name}", r, t)
            print(line)
            assert RC.passes(r), line
            for k in r:
                worst[k], beside[k] = max(worst.get(k, 0.0), r[k]), max(beside.get(k, 0.0), t[k])
            # the same bits whichever taps are taken
            only_s = _run(model, images, hooks, names_filter=pre + "hook_scale")
            only_n = _run(model, images, hooks, names_filter=pre + "hook_normalized")
            assert list(only_s) == [pre + "hook_scale"] and list(only_n) == [pre + "hook_normalized"]
            assert _same_bits(only_s[pre + "hook_scale"], scale), name
            assert _same_bits(only_n[pre + "hook_normalized"], norm), name
    print(RC.report(f"WORST {_name(dtype)} d={d} {ENTRY[d]}", worst, beside))


# --------------------------------------------------------------------------------------------------------------------- EMBED form
@functools.lru_cache(maxsize=None)
def _embed_model(dtype, d, layer_norm_pre=True):
    model = _vit(dtype, d, 1, 64, layer_norm_pre=layer_norm_pre)
    x = torch.randn(B, 3, 8, 8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(d + 1)).to(dtype)
    return model, x


def _plant_embed(model, name, d, dtype):
    """W_pos = rows 0 .. 4 of the case, cls token = row 5, conv bias = row 7, conv weight 0 (rows 1 and 6 are the bad ones of
    ``nonfinite``: token 1 of every image is bad, every workgroup keeps good rows).  Returns the rows [B * T, d] the kernel must build:
    (cls | bias) + pos in the storage dtype's arithmetic -- an fp32 sum, rounded once in bf16 mode."""
    rows = RC.ln_rows(name, 8, d)
    pos, cls, bias = rows[:T], rows[5], rows[7]
    with torch.no_grad():
        model.pos_embed.W_pos.copy_(pos.to(dtype))
        model.cls_token.copy_(cls.view(1, 1, d).to(dtype))
        model.embed.proj.weight.zero_()
        model.embed.proj.bias.copy_(bias.to(dtype))
    model.invalidate_native_weights()
    e = torch.cat([cls[None], bias[None].expand(T - 1, d)])                       # [T, d]
    x = (e + pos).to(dtype).float()
    return x[None].expand(B, T, d).reshape(B * T, d).contiguous(), bias


@pytest.mark.parametrize("d", [136, 520, 2048])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_name)
def test_embed_form_of_layer_norm_on_planted_rows(dtype, d):
    bf16 = dtype == BF16
    model, images = _embed_model(dtype, d)
    worst, beside = {}, {}
    for planted in (True, False):
        w, b = RC.ln_weights(d, planted)
        _plant_ln_weights(model, w, b)
        for name in RC.LN_CASES:
            x, bias = _plant_embed(model, name, d, dtype)
            cache = _run(model, images)
            assert _same(cache["hook_embed"], bias[None, None].expand(B, T - 1, d)), name
            full = cache["hook_full_embed"]
            assert full.dtype == dtype and _same(full, x.view(B, T, d)), (name, "hook_full_embed is not round(e + pos)")
            scale, norm, out = cache["ln_pre.hook_scale"], cache["ln_pre.hook_normalized"], cache["hook_ln_pre"]
            assert scale.dtype == norm.dtype == F32 and out.dtype == dtype
            assert _same_bits(out, norm.to(dtype)), (name, "hook_ln_pre is not the fp32 tap in the storage dtype")
            r = RC.check_ln(x, w, b, scale=scale.cpu().view(-1), y32=norm.cpu().view(-1, d), y16=out.cpu().view(-1, d) if bf16 else None)
            t = RC.ln_torch_ratios(x, w, b, bf16=bf16)
            line = RC.report(f"{_name(dtype)} d={d} EMBED {'planted' if planted else 'default'} w, b  {name}", r, t)
            print(line)
            assert RC.passes(r), line
            for k in r:
                worst[k], beside[k] = max(worst.get(k, 0.0), r[k]), max(beside.get(k, 0.0), t[k])
            only_s = _run(model, images, names_filter="ln_pre.hook_scale")
            only_n = _run(model, images, names_filter="ln_pre.hook_normalized")
            assert _same_bits(only_s["ln_pre.hook_scale"], scale) and _same_bits(only_n["ln_pre.hook_normalized"], norm), name
    print(RC.report(f"WORST {_name(dtype)} d={d} EMBED", worst, beside))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_name)
def test_embed_form_without_ln_pre_still_writes_hook_full_embed(dtype):
    """layer_norm_pre = False: ln_kernel<T, true> leaves at ``do_ln = 0`` with hook_full_embed (= block 0's hook_resid_pre) written"""
    d = 520
    model, images = _embed_model(dtype, d, False)
    for name in RC.LN_CASES:
        x, _ = _plant_embed(model, name, d, dtype)
        cache = _run(model, images, names_filter=lambda n: n in ("hook_full_embed", "blocks.0.hook_resid_pre"))
        assert sorted(cache) == ["blocks.0.hook_resid_pre", "hook_full_embed"]
        assert cache["hook_full_embed"].dtype == dtype and _same(cache["hook_full_embed"], x.view(B, T, d)), name
        assert _same(cache["blocks.0.hook_resid_pre"], x.view(B, T, d)), name


# ------------------------------------------------------------------------------------------------------------ fused activation
N_ACT = 256


def _values(dtype, which):
    """65 536 pre-activations: the finite bf16 values padded with repeats, or fp32 values that are no bf16 values"""
    if which == "bf16":
        v = RC.finite_bf16().float()
        return torch.cat([v, v[: N_ACT * N_ACT - v.numel()]])
    assert dtype == F32
    return RC.fp32_extra(N_ACT * N_ACT)


_FUSED = {}


def _fused(dtype, act, tile, which, pre_tap=True):
    """(out0, out1) [256, 256] of the ACT epilogue on value (256 m + n) at [m][n]; computed once per setting"""
    key = (dtype, act, tile, which, pre_tap)
    if key in _FUSED:
        return _FUSED[key]
    _native.set_tuning("reset")
    if tile is not None:
        _native.set_tuning("gemm_tile", tile)
    try:
        n = N_ACT
        vals = _values(dtype, which).to(dtype).cuda()
        A = torch.eye(n, device="cuda", dtype=dtype)
        Bt = vals.view(n, n).t().contiguous()                                    # B[n][k] = value 256 k + n
        bias = torch.zeros(n, device="cuda", dtype=dtype)
        o0 = torch.full((n + 1, n), 7.0, device="cuda", dtype=dtype) if pre_tap else None
        o1 = torch.full((n + 1, n), 7.0, device="cuda", dtype=dtype)
        L = _native.lib()
        _native.check(L.pv_gemm_epilogue(1 if dtype == BF16 else 0, 3, RC.PV_ACT[act], A.data_ptr(), n, Bt.data_ptr(), n, bias.data_ptr(),
                                         None, n, o0.data_ptr() if pre_tap else None, o1.data_ptr(), n, n, n, n,
                                         torch.cuda.current_stream().cuda_stream), "pv_gemm_epilogue")
        torch.cuda.synchronize()
        for o in (o0, o1):
            assert o is None or bool((o[n].float() == 7.0).all())                # the row behind the last stays untouched
    finally:
        _native.set_tuning("reset")
    _FUSED[key] = (None if o0 is None else o0[:n].cpu(), o1[:n].cpu())
    return _FUSED[key]


@pytest.mark.parametrize("act", RC.ACTS)
def test_fused_activation_over_every_finite_bf16_value(act, tuning):
    vals = _values(BF16, "bf16")
    outs = {tile: _fused(BF16, act, tile, "bf16") for tile in (0, 4, 5)}
    o0, o1 = outs[0]
    assert o0.dtype == o1.dtype == BF16 and _same(o0.view(-1), vals), "out0 is not the planted value"
    r = RC.check_act(act, True, o0.view(-1).float(), o1.view(-1))
    t = RC.act_torch_ratio(act, True, vals[vals < RC.TORCH_GELU_MAX] if act == "gelu" else vals)
    line = RC.report(f"fused bf16 {act}, all finite bf16", r, t)
    print(line)
    assert RC.passes(r), line
    for tile in (4, 5):
        assert _same(outs[tile][0].view(-1), vals), tile
        assert torch.equal(outs[tile][1].view(torch.int16), o1.view(torch.int16)), (tile, "out1 differs between the GEMM kernels")
    for tile in (0, 4, 5):                                                       # without the pre-activation tap (out0 = NULL)
        assert torch.equal(_fused(BF16, act, tile, "bf16", pre_tap=False)[1].view(torch.int16), o1.view(torch.int16)), tile


@pytest.mark.parametrize("which", ["bf16", "extra"])
@pytest.mark.parametrize("act", RC.ACTS)
def test_fused_activation_fp32(act, which, tuning):
    vals = _values(F32, which)
    o0, o1 = _fused(F32, act, None, which)
    assert o0.dtype == o1.dtype == F32 and _same(o0.view(-1), vals), "out0 is not the planted value"
    r = RC.check_act(act, False, o0.view(-1), o1.view(-1))
    t = RC.act_torch_ratio(act, False, vals[vals < RC.TORCH_GELU_MAX] if act == "gelu" else vals)
    line = RC.report(f"fused fp32 {act}, {'all finite bf16' if which == 'bf16' else 'fp32_extra'}", r, t)
    print(line)
    assert RC.passes(r), line
    assert torch.equal(_fused(F32, act, None, which, pre_tap=False)[1].view(torch.int32), o1.view(torch.int32))


# ------------------------------------------------------------------------------------------------------ stand-alone activation
ACT_B, ACT_T, ACT_DMLP = 2, 17, 2048                     # 69 632 elements


@functools.lru_cache(maxsize=None)
def _act_model(dtype, act):
    model = _vit(dtype, 64, 1, ACT_DMLP, image_size=16, activation=act, n_heads=2)
    assert model.n_tokens == ACT_T
    x = torch.randn(ACT_B, 3, 16, 16, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)).to(dtype)
    return model, x


@pytest.mark.parametrize("act", RC.ACTS)
@pytest.mark.parametrize("dtype,which", [(F32, "bf16"), (F32, "extra"), (BF16, "bf16")], ids=["fp32-bf16", "fp32-extra", "bf16-bf16"])
def test_stand_alone_activation_behind_a_hook_on_mlp_pre(dtype, which, act, tuning):
    bf16 = dtype == BF16
    n = ACT_B * ACT_T * ACT_DMLP
    if which == "bf16":
        allv = RC.all_bf16().float()                                             # every bit pattern, NaN and +-inf included
        pre = torch.cat([allv, allv[: n - allv.numel()]])
    else:
        extra = RC.fp32_extra(N_ACT * N_ACT)
        pre = torch.cat([extra, extra[: n - extra.numel()]])
    plant = pre.view(ACT_B, ACT_T, ACT_DMLP).to(dtype).cuda()
    model, images = _act_model(dtype, act)
    key = "blocks.0.mlp.hook_"
    cache = _run(model, images, [(key + "pre", lambda t, hook=None: plant)], names_filter=lambda s: s.startswith(key))
    assert _same(cache[key + "pre"], plant)
    post = cache[key + "post"].cpu().view(-1)
    assert post.dtype == dtype
    r = RC.check_act(act, bf16, pre, post)
    fin = torch.isfinite(pre) & ((pre < RC.TORCH_GELU_MAX) | (act != "gelu"))
    t = RC.act_torch_ratio(act, bf16, pre[fin])
    line = RC.report(f"stand-alone {_name(dtype)} {act}, {'all 65 536 bf16 patterns' if which == 'bf16' else 'fp32_extra'}", r, t)
    print(line)
    assert RC.passes(r), line
    # the bits of the fused epilogue (csrc/gemm.hpp: pv_launch_act is the instruction sequence of the GEMM epilogues)
    fused_in, fused_out = _values(dtype, which), _fused(dtype, act, 0 if bf16 else None, which)[1].view(-1)
    as_int = torch.int16 if bf16 else torch.int32
    if which == "bf16":
        table = torch.zeros(65536, dtype=torch.int64)                            # bf16 bit pattern -> bits of the fused result
        idx = fused_in.to(BF16).view(torch.int16).long() & 0xFFFF
        table[idx] = fused_out.view(as_int).long()
        finite = torch.isfinite(pre) & (pre != 0)                                # (the GEMM's acc + bias turns a planted -0 into +0)
        want = table[pre.to(BF16).view(torch.int16).long() & 0xFFFF]
        got = post.view(as_int).long()
        assert bool((got == want)[finite].all()), "the stand-alone kernel and the fused epilogue differ"
        assert bool((post[pre == 0] == 0).all())
    else:
        m = fused_in.numel()
        assert torch.equal(post[:m].view(as_int), fused_out.view(as_int)), "the stand-alone kernel and the fused epilogue differ"
