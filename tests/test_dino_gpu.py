"""The DINO family on the HIP plan: attention for 640 < T <= 2048 in every (dtype, d_head) the plan supports, the resumed attention
core at those lengths, the pooled final stages ("gaap", the dino-vitb concatenation) and the dino-vits8 configuration end to end.
Run with ``-m gpu`` on an MI355X.

Attention bounds are those of test_native_vit_gpu.test_bf16_long_sequence_attention_kernel -- against an fp32 recompute from the
q, k, v the same run cached: bf16 ``2^-8 max|ref| + 1e-6`` for scores and z and ``2^-8`` absolute for the pattern (one bf16 rounding of a
value <= max|ref| resp. <= 1), fp32 ``rel_fro < FP32_TOL``; the pattern also per element (bf16 ``2^-8 ref + 1e-30``) resp. per row (fp32).  Token counts (patch 4): 677 (just past the old cap; the last 32-key tile
holds 5 keys), 785 (DINO /8), 1025 (one key past a tile edge), 2026 (at the cap).
"""
import os

import numpy as np
import pytest
import torch

from vit_prisma_amd import HookedViT, HookedViTConfig
from vit_prisma_amd.synth import synth_images

import _rowop_cases as RC
from _attention_cases import pattern_elementwise_ok
from test_dino_cpu import GOLDEN, POOLED_ARCHS, POOLED_BATCH, POOLED_KEYS, pooled_model, rel_fro

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4
BF16_EPS = 2.0 ** -8
SIZES = {104: 677, 112: 785, 128: 1025, 180: 2026}


def long_model(dtype, d_head, image_size):
    cfg = dict(n_layers=1, d_model=2 * d_head, n_heads=2, d_head=d_head, d_mlp=128, patch_size=4, image_size=image_size, n_channels=3,
               n_classes=16, eps=1e-5, layer_norm_pre=True, normalize_output=True, return_type="class_logits", activation_name="gelu",
               use_cls_token=True, normalization_type="LN", classification_type="cls")
    torch.manual_seed(image_size + d_head)
    model = HookedViT(HookedViTConfig(**cfg, dtype=dtype, device="cuda")).to(dtype).cuda().eval().use_native(True)
    x = torch.randn(2, 3, image_size, image_size, device="cuda", generator=torch.Generator(device="cuda").manual_seed(image_size)).to(dtype)
    return model, x


def close(got, ref, dtype, what, absolute=False):
    """The issue's bounds: fp32 rel_fro < FP32_TOL; bf16 2^-8 max|ref| + 1e-6 (``absolute``: 2^-8, the pattern's)."""
    got, ref = got.float(), ref.float()
    if dtype == torch.float32:
        err, bound = rel_fro(got, ref), FP32_TOL
    else:
        err = float((got - ref).abs().max())
        bound = BF16_EPS if absolute else BF16_EPS * float(ref.abs().max()) + 1e-6
    print(f"{what}: {err:.3e} (bound {bound:.3e})")
    assert (err < bound) if dtype == torch.float32 else (err <= bound), (what, err, bound)
    if absolute:
        # the pattern also per element / per row (tests/_attention_cases.py): at these T every element is below 2^-8, so the absolute
        # bound alone passes an all-zero pattern.  bf16: 2^-8 ref + 1e-30 per element; fp32: relative L2 of each row < FP32_TOL
        if dtype == torch.float32:
            num, den = (got - ref).double().pow(2).sum(-1).sqrt(), ref.double().pow(2).sum(-1).sqrt()
            worst = float((num / den.clamp_min(1e-300)).max())
            print(f"{what}: worst row {worst:.3e} (bound {FP32_TOL:.3e})")
            assert worst < FP32_TOL and bool((got[den == 0] == 0).all()), (what, worst)
        else:
            ok, worst = pattern_elementwise_ok(got, ref)
            print(f"{what}: worst element error / (2^-8 ref + 1e-30) = {worst:.4f}")
            assert ok, (what, worst)


def check_attention(model, x, dtype, d_head, T):
    with torch.no_grad():
        _, cache = model.run_with_cache(x)
        assert model.last_run_native
        _, only_z = model.run_with_cache(x, names_filter="blocks.0.attn.hook_z")                                       # no taps at all
        assert model.last_run_native
        _, pat_z = model.run_with_cache(x, names_filter=lambda n: n.endswith(("attn.hook_pattern", "attn.hook_z")))  # no score tap
        assert model.last_run_native
    q, k, v = (cache["blocks.0.attn." + n].float() for n in ("hook_q", "hook_k", "hook_v"))
    s_ref = torch.einsum("bqhd,bkhd->bhqk", q, k) / (d_head ** 0.5)
    s_got = cache["blocks.0.attn.hook_attn_scores"]
    assert s_got.shape == (2, 2, T, T) and s_got.dtype == dtype
    close(s_got, s_ref, dtype, "scores")
    p_ref = torch.softmax(s_got.float(), dim=-1)
    p_got = cache["blocks.0.attn.hook_pattern"]
    assert p_got.shape == (2, 2, T, T) and p_got.dtype == dtype
    close(p_got, p_ref, dtype, "pattern", absolute=True)
    z_ref = torch.einsum("bhqk,bkhd->bqhd", p_got.float(), v)
    close(cache["blocks.0.attn.hook_z"], z_ref, dtype, "z")
    # without the score tap: the same statements, and the same z whichever taps are taken
    close(pat_z["blocks.0.attn.hook_pattern"], p_ref, dtype, "pattern (no score tap)", absolute=True)
    assert torch.equal(only_z["blocks.0.attn.hook_z"], cache["blocks.0.attn.hook_z"])
    assert torch.equal(pat_z["blocks.0.attn.hook_z"], cache["blocks.0.attn.hook_z"])
    assert torch.equal(pat_z["blocks.0.attn.hook_pattern"], p_got)


@pytest.mark.parametrize("image_size", sorted(SIZES))
@pytest.mark.parametrize("dtype,d_head", [(torch.float32, 32), (torch.float32, 64), (torch.bfloat16, 32), (torch.bfloat16, 64)],
                         ids=["fp32-dh32", "fp32-dh64", "bf16-dh32", "bf16-dh64"])
def test_long_sequence_attention(dtype, d_head, image_size):
    model, x = long_model(dtype, d_head, image_size)
    check_attention(model, x, dtype, d_head, SIZES[image_size])


@pytest.mark.parametrize("image_size", [104, 180])
def test_attn_wg_override_selects_the_streaming_kernel_beyond_640(tuning, image_size):
    """bf16 / d_head 64 normally runs attn_lean_kernel; with attn_wg = 1 the workgroup kernel's LDS strip cannot hold T > 640 and the
    streaming kernel must serve it (it used to be an error)."""
    model, x = long_model(torch.bfloat16, 64, image_size)
    tuning("attn_wg", 1)
    check_attention(model, x, torch.bfloat16, 64, SIZES[image_size])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_hooked_scores_with_nan_and_all_minus_inf_rows_at_677(dtype):
    """A hook on hook_attn_scores (the resumed attention core, one wave per row, at T = 677): a row holding a NaN and a row of nothing
    but -inf come back as exact zeros (attention.py:148-150), every other row is softmax of the edited scores."""
    T = 677
    model, x = long_model(dtype, 32, 104)

    def edit(t, hook=None):
        t = t.clone()
        t[0, 1, 5, 300] = float("nan")
        t[1, 0, 650, :] = float("-inf")
        return t

    with torch.no_grad():
        _, plain = model.run_with_cache(x, names_filter=lambda n: n.endswith(("hook_attn_scores", "hook_v")))
        _, cache = model.run_with_cache(x, fwd_hooks=[("blocks.0.attn.hook_attn_scores", edit)])
    assert model.last_run_native, model.native_fallback_reason
    p_got = cache["blocks.0.attn.hook_pattern"]
    assert p_got.shape == (2, 2, T, T)
    assert float(p_got[0, 1, 5].abs().max()) == 0.0 and float(p_got[1, 0, 650].abs().max()) == 0.0
    p_ref = torch.softmax(edit(plain["blocks.0.attn.hook_attn_scores"]).float(), dim=-1)
    p_ref = torch.where(torch.isnan(p_ref), torch.zeros_like(p_ref), p_ref)
    assert float(p_ref[0, 1, 5].abs().max()) == 0.0 and float(p_ref[1, 0, 650].abs().max()) == 0.0
    close(p_got, p_ref, dtype, "pattern behind the hook", absolute=True)
    z_ref = torch.einsum("bhqk,bkhd->bqhd", p_got.float(), plain["blocks.0.attn.hook_v"].float())
    close(cache["blocks.0.attn.hook_z"], z_ref, dtype, "z behind the hook")
    assert float(cache["blocks.0.attn.hook_z"][0, 5, 1].abs().max()) == 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_hooked_pattern_at_785(dtype):
    """A hook on hook_pattern that zeroes the last key column: z is the edited pattern times v."""
    model, x = long_model(dtype, 32, 112)

    def edit(t, hook=None):
        t = t.clone()
        t[..., -1] = 0
        return t

    with torch.no_grad():
        _, plain = model.run_with_cache(x, names_filter=lambda n: n.endswith(("hook_pattern", "hook_v")))
        _, cache = model.run_with_cache(x, fwd_hooks=[("blocks.0.attn.hook_pattern", edit)])
    assert model.last_run_native, model.native_fallback_reason
    z_ref = torch.einsum("bhqk,bkhd->bqhd", edit(plain["blocks.0.attn.hook_pattern"]).float(), plain["blocks.0.attn.hook_v"].float())
    close(cache["blocks.0.attn.hook_z"], z_ref, dtype, "z behind the pattern hook")


@pytest.mark.parametrize("tag", sorted(POOLED_ARCHS))
def test_pooled_heads_natively_vs_reference_fixture_fp32(tag):
    G = np.load(os.path.join(GOLDEN, "vit_tiny_pooled_heads.npz"))
    model = pooled_model(tag, torch.float32, "cuda").use_native(True)
    x = torch.from_numpy(synth_images(POOLED_ARCHS[tag], POOLED_BATCH, 1)).cuda()
    with torch.no_grad():
        out, cache = model.run_with_cache(x)
        plain = model(x)
    assert model.last_run_native, model.native_fallback_reason
    want = torch.from_numpy(G[f"{tag}::__out__"])
    assert out.shape == want.shape and plain.shape == want.shape
    assert list(cache.keys()) == list(G[f"{tag}::__keys__"])
    assert rel_fro(out.cpu(), want) < FP32_TOL and rel_fro(plain.cpu(), want) < FP32_TOL
    for k in POOLED_KEYS:
        assert cache[k].shape == G[f"{tag}::{k}"].shape, k
        assert rel_fro(cache[k].cpu(), torch.from_numpy(G[f"{tag}::{k}"])) < FP32_TOL, k


def check_pooled_vector(model, x, tag, dtype):
    """hook_post_head_pre_normalize of a head-less model IS the pooled vector: against an fp32 mean of the hook_ln_final the same run
    cached -- one rounding of an fp32-accumulated mean: 2^-8 max|x| + 1e-6 in bf16, FP32_TOL in fp32; the CLS half is a copy."""
    with torch.no_grad():
        out, cache = model.run_with_cache(x)
    assert model.last_run_native, model.native_fallback_reason
    lnf, pooled = cache["hook_ln_final"].float(), cache["hook_post_head_pre_normalize"]
    B, T, d = lnf.shape
    if tag == "gaap":
        assert pooled.shape == (B, d)
        close(pooled, lnf.mean(dim=1), dtype, "mean over all tokens")
        want_out = torch.nn.functional.normalize(pooled.float(), dim=-1)
    else:
        assert pooled.shape == (B, d, 2) and out.shape == (B, d, 2)
        assert torch.equal(pooled[..., 0], cache["hook_ln_final"][:, 0])
        close(pooled[..., 1], lnf[:, 1:].mean(dim=1), dtype, "mean over the patch tokens")
        want_out = torch.nn.functional.normalize(pooled.float(), dim=-1)
    close(out, want_out, dtype, "normalised output")
    # per column / per element (tests/_rowop_cases.py): the float64 mean of the cached hook_ln_final, the float64 normalise of the pooled vector
    bf16 = dtype == torch.bfloat16
    t0 = 0 if tag == "gaap" else 1
    r_mean = RC.check_token_mean(cache["hook_ln_final"].cpu(), (pooled if tag == "gaap" else pooled[..., 1]).cpu(), t0, bf16)
    r_norm = RC.check_l2norm(pooled.cpu().reshape(-1, pooled.shape[-1]), out.cpu().reshape(-1, pooled.shape[-1]), bf16)
    print(f"{tag} d_model {d} T {T}: error / bound  token mean {r_mean:.3g}  l2 normalise {r_norm:.3g}")
    assert r_mean <= 1.0 and r_norm <= 1.0, (tag, d, T, r_mean, r_norm)


@pytest.mark.parametrize("tag", sorted(POOLED_ARCHS))
def test_pooled_vector_bf16(tag):
    model = pooled_model(tag, torch.bfloat16, "cuda", return_type="pre_logits").use_native(True)
    x = torch.from_numpy(synth_images(POOLED_ARCHS[tag], POOLED_BATCH, 1)).cuda().bfloat16()
    check_pooled_vector(model, x, tag, torch.bfloat16)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_dino_vitb_pooling_meets_long_attention_at_785(dtype):
    torch.manual_seed(785)
    model = pooled_model("dino", dtype, "cuda", image_size=112, patch_size=4).use_native(True)
    assert model.n_tokens == 785
    x = torch.randn(2, 3, 112, 112, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7)).to(dtype)
    check_pooled_vector(model, x, "dino", dtype)


def wide_pooled_model(tag, dtype, d_model, image_size, cls, n_layers):
    """a head-less pooled model at a d_model beyond one 128-column workgroup of token_mean_kernel (patch 4)"""
    cfg = dict(n_layers=n_layers, d_model=d_model, n_heads=2, d_head=32, d_mlp=64, patch_size=4, image_size=image_size, n_channels=3,
               n_classes=16, eps=1e-5, layer_norm_pre=True, normalize_output=True, return_type="pre_logits", activation_name="gelu",
               use_cls_token=cls, normalization_type="LN", classification_type="gaap" if tag == "gaap" else "cls",
               model_name="synthetic-wide-gaap" if tag == "gaap" else "facebook/dino-vitb-wide")
    torch.manual_seed(d_model + image_size)
    model = HookedViT(HookedViTConfig(**cfg, dtype=dtype, device="cuda")).to(dtype).cuda().eval().use_native(True)
    with torch.no_grad():                                 # (an ln_final away from the identity, so that the columns differ in size)
        model.ln_final.w.copy_(RC.ln_weights(d_model)[0].to(dtype))
        model.ln_final.b.copy_(RC.ln_weights(d_model)[1].to(dtype))
    x = torch.randn(POOLED_BATCH, 3, image_size, image_size, device="cuda",
                    generator=torch.Generator(device="cuda").manual_seed(d_model)).to(dtype)
    return model, x


# token_mean_kernel: a workgroup owns 128 columns (a lane two), wave w the tokens t0 + w, t0 + w + 4, ...
#   d_model 136   two workgroups in x, the second with 4 active lanes          d_model 264   three, the last with 4 active lanes
#   T = 17        every wave has tokens                                        T - t0 = 1, 2  three / two waves have none: "gaap" without
#   a cls token at one patch (T = 1), with it (T = 2); the dino concatenation at one patch (T = 2, t0 = 1).  T - t0 = 3 does not exist
#   on a square patch grid.  The few-token models have no blocks (n_layers = 0): ln_final reads the embedding stage's output.
WIDE = [(tag, d, 16, True, 1) for tag in ("gaap", "dino") for d in (136, 264)] + \
       [("gaap", 264, 4, False, 0), ("gaap", 136, 4, True, 0), ("dino", 264, 4, True, 0)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("tag,d_model,image_size,cls,n_layers", WIDE,
                         ids=[f"{w[0]}-d{w[1]}-T{(w[2] // 4) ** 2 + int(w[3])}" for w in WIDE])
def test_pooled_vector_beyond_one_workgroup_and_with_idle_waves(tag, d_model, image_size, cls, n_layers, dtype):
    model, x = wide_pooled_model(tag, dtype, d_model, image_size, cls, n_layers)
    assert model.n_tokens == (image_size // 4) ** 2 + int(cls)
    check_pooled_vector(model, x, tag, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("n_classes", [16, 136, 1000])
def test_l2_normalise_per_row_ragged_workgroup_and_a_zero_row(n_classes, batch, dtype):
    """l2norm_kernel on the head's output: rows = B in {1, 5} (a 4-row workgroup with 1 row; one full and one with 1), row lengths 16
    (a quarter of the lanes), 136 and 1000 (no multiple of 64), every element against float64 x / max(||x||, 1e-12).  At B = 5 image 2
    is handed a constant CLS row by a hook on the last hook_resid_post: with ln_final.b = 0 its LayerNorm is exactly 0, the head (b_H =
    0) gives an all-zero row, and that row must stay zero."""
    cfg = dict(n_layers=1, d_model=64, n_heads=2, d_head=32, d_mlp=64, patch_size=4, image_size=8, n_channels=3, n_classes=n_classes,
               eps=1e-5, layer_norm_pre=True, normalize_output=True, return_type="class_logits", activation_name="gelu",
               use_cls_token=True, normalization_type="LN", classification_type="cls")
    torch.manual_seed(n_classes)
    model = HookedViT(HookedViTConfig(**cfg, dtype=dtype, device="cuda")).to(dtype).cuda().eval().use_native(True)
    with torch.no_grad():
        model.ln_final.b.zero_()
        model.head.b_H.zero_()
    x = torch.randn(batch, 3, 8, 8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(batch)).to(dtype)
    zero_row = 2 if batch == 5 else None

    def flatten_cls(t, hook=None):
        t = t.clone()
        if zero_row is not None:
            t[zero_row, 0, :] = 1.5
        return t

    with torch.no_grad():
        out, cache = model.run_with_cache(x, fwd_hooks=[("blocks.0.hook_resid_post", flatten_cls)])
    assert model.last_run_native, model.native_fallback_reason
    head = cache["hook_post_head_pre_normalize"]
    assert head.shape == out.shape == (batch, n_classes) and out.dtype == dtype
    if zero_row is not None:
        assert float(head[zero_row].abs().max()) == 0.0 and float(out[zero_row].abs().max()) == 0.0
        assert float(head[[0, 1, 3, 4]].float().abs().amax(-1).min()) > 0.0
    r = RC.check_l2norm(head.cpu(), out.cpu(), dtype == torch.bfloat16)
    print(f"l2 normalise {n_classes} x {batch}: error / bound {r:.3g} ({RC.l2norm_units(n_classes):.1f} u)")
    assert r <= 1.0, r
    close(out, torch.nn.functional.normalize(head.float(), dim=-1), dtype, "normalised output")


def test_hook_on_ln_final_of_dino_vitb_gives_the_pytorch_answer():
    """A hook on hook_ln_final puts the final stage on the model's own modules (split_plan): it must build the same [B, d, 2]
    concatenation as HookedViT.forward does."""
    model = pooled_model("dino", torch.float32, "cuda").use_native(True)
    x = torch.from_numpy(synth_images(POOLED_ARCHS["dino"], POOLED_BATCH, 1)).cuda()
    seen = []

    def look(t, hook=None):
        seen.append(tuple(t.shape))
        return t

    with torch.no_grad():
        out = model.run_with_hooks(x, fwd_hooks=[("hook_ln_final", look)])
        assert model.last_run_native, model.native_fallback_reason
        model.use_native(False)
        want = model.run_with_hooks(x, fwd_hooks=[("hook_ln_final", look)])
    assert seen == [(POOLED_BATCH, 17, 64)] * 2
    assert out.shape == want.shape == (POOLED_BATCH, 64, 2)
    assert rel_fro(out, want) < FP32_TOL


def test_dino_vits8_all_hooks_natively_same_keys_and_shapes_as_pytorch():
    from vit_prisma_amd.model_loader import load_config
    cfg = load_config("facebook/dino-vits8", dtype=torch.bfloat16, device="cuda")
    torch.manual_seed(8)
    model = HookedViT(cfg).to(torch.bfloat16).cuda().eval().use_native(True)
    assert model.n_tokens == 785
    x = torch.randn(2, 3, 224, 224, device="cuda", generator=torch.Generator(device="cuda").manual_seed(8)).bfloat16()
    with torch.no_grad():
        out, cache = model.run_with_cache(x)
        assert model.last_run_native, model.native_fallback_reason
        model.use_native(False)
        out_t, cache_t = model.run_with_cache(x)
        assert not model.last_run_native
    assert out.shape == out_t.shape == (2, 384)
    assert list(cache.keys()) == list(cache_t.keys()) and len(cache.keys()) > 12 * 17
    for k in cache_t.keys():
        assert cache[k].shape == cache_t[k].shape and cache[k].dtype == cache_t[k].dtype, k
    assert bool(torch.isfinite(out.float()).all())
