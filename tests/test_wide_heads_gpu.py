"""Wide heads on the HIP plan: ``attn_wide_kernel`` (csrc/attention_wide.hip; its body: csrc/attn_stream.hpp) and the resumed attention core at 64 < d_head <= 128.
Run with ``-m gpu`` on an MI355X.

The row that the dispatch table in test_attention_adversarial_gpu.py cannot get (pv_launch_attention sends these shapes to their
launcher BEFORE dispatch_attn, at every T, whatever the attn_wg override says):

    fp32 / bf16, 64 < d_head <= 128, d_head % 8 == 0, T <= 2048
        d_head  72 -  96   attn_wide_kernel<.., 96>     fp32 and bf16, dh 80 (a whole zero k-step of the bf16 MFMA), 88 (an odd
                                                        number of 16-byte chunks in bf16)
        d_head 104 - 128   attn_wide_kernel<.., 128>    fp32 and bf16, dh 104 (padded), 128 (no padding; sqrt(128) is no power of two
                                                        either: the division form)
        each at T = 17 (odd, less than one key tile), 65 (one key into the third tile), 257 (these models' own T), 677 (past 640, a
        ragged last tile of 5 keys; two 128-query blocks at 257, six at 677, the last one with idle waves)

(a) the adversarial q, k, v of tests/_attention_cases.py, handed in by hooks exactly as test_attention_adversarial_gpu.py does, with that
    module's derived bounds: bf16 at one rounding (2^-8, per element for the pattern), fp32 at 1e-4 relative L2 per row.  A float32
    torch twin (scores round(q k / sqrt(dh)), torch softmax, rounded) stays inside them on the CPU for every dh in {72, ..., 128}, every
    T here, all three cases and both dtypes (worst ratio bf16 0.996, fp32 0.0076), so no element is excluded.
(b) B H = 4 in (a) leaves the per-XCD remap of whole heads off: a recompute check (test_dino_gpu's bounds) at 3 images x 3 heads of 80
    (one whole round of 8 plus a remainder), and one layer of ViT-H/14's true geometry (16 heads of 80, T = 257, batch 2, bf16).
(c) the tiny wide model against the reference's own run (tests/golden/vit_tiny_wide.npz) in fp32; in bf16 by the rule of
    test_native_vit_gpu's ``held`` (error against the fp32 run <= INTRA_BLOCK_RATIO x the PyTorch bf16 path's own), and scores, pattern
    and z by the recompute bounds of (b).
(d) hooks on hook_attn_scores (a NaN row, an all -inf row), hook_pattern and hook_z: the resumed attention core with d = lane, lane + 64.
(e) use_attn_result: the derived attn.hook_result entry.
"""
import functools
import os

import numpy as np
import pytest
import torch

from vit_prisma_amd import HookedViT, HookedViTConfig
from vit_prisma_amd.synth import ARCHS, synth_images

import _attention_cases as AC
from test_dino_gpu import BF16_EPS, FP32_TOL, close
from test_native_vit_gpu import INTRA_BLOCK_RATIO, _pytorch_twin
from test_wide_heads_cpu import GOLDEN, WIDE_BATCH, rel_fro, wide_tiny_model

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
IMAGE = {17: 16, 65: 32, 257: 64, 677: 104}                       # T -> image size at patch 4, with a cls token
PATHS = [(dt, dh, T) for dt in (F32, BF16) for dh in (80, 88, 104, 128) for T in sorted(IMAGE)]


def _id(path):
    dtype, dh, T = path
    return f"wide{96 if dh <= 96 else 128}-{'bf16' if dtype == BF16 else 'fp32'}-dh{dh}-T{T}"


def _build(dtype, d_model, n_heads, d_head, d_mlp, patch, image_size, seed, **kw):
    cfg = dict(n_layers=1, d_model=d_model, n_heads=n_heads, d_head=d_head, d_mlp=d_mlp, patch_size=patch, image_size=image_size,
               n_channels=3, n_classes=16, eps=1e-5, layer_norm_pre=True, normalize_output=True, return_type="class_logits",
               activation_name="gelu", use_cls_token=True, normalization_type="LN", classification_type="cls")
    cfg.update(kw)
    torch.manual_seed(seed)
    return HookedViT(HookedViTConfig(**cfg, dtype=dtype, device="cuda")).to(dtype).cuda().eval().use_native(True)


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) adversarial inputs
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model(dtype, dh, T):
    model = _build(dtype, 2 * dh, 2, dh, 128, 4, IMAGE[T], T + dh)
    assert model.n_tokens == T
    x = torch.randn(AC.B, 3, IMAGE[T], IMAGE[T], device="cuda", generator=torch.Generator(device="cuda").manual_seed(T)).to(dtype)
    return model, x


@functools.lru_cache(maxsize=None)
def _case(name, T, dh):
    return tuple(t.cuda() for t in AC.make_case(name, T, dh))


@pytest.mark.parametrize("name", AC.CASES)
@pytest.mark.parametrize("path", PATHS, ids=_id)
def test_wide_attention_kernel_on_adversarial_inputs(path, name):
    dtype, dh, T = path
    model, x = _model(dtype, dh, T)
    q, k, v = _case(name, T, dh)
    pre = "blocks.0.attn."
    hooks = [(pre + n, (lambda t, hook=None, r=r.to(dtype): r)) for n, r in (("hook_q", q), ("hook_k", k), ("hook_v", v))]
    with torch.no_grad():
        _, cache = model.run_with_cache(x, fwd_hooks=hooks)                                              # every tap
        assert model.last_run_native, model.native_fallback_reason
        _, pat_z = model.run_with_cache(x, fwd_hooks=hooks, names_filter=lambda n: n.endswith(("attn.hook_pattern", "attn.hook_z")))
        assert model.last_run_native, model.native_fallback_reason
        _, only_z = model.run_with_cache(x, fwd_hooks=hooks, names_filter=pre + "hook_z")                  # no tap at all
        assert model.last_run_native, model.native_fallback_reason
    for n, r in (("hook_q", q), ("hook_k", k), ("hook_v", v)):      # the kernel was handed these values, bit for bit
        got = cache[pre + n]
        assert got.dtype == dtype and bool(((got.float() == r) | (torch.isnan(got) & torch.isnan(r))).all()), n
    s_got, p_got, z_got = (cache[pre + n] for n in ("hook_attn_scores", "hook_pattern", "hook_z"))
    assert s_got.shape == p_got.shape == (AC.B, AC.H, T, T) and z_got.shape == (AC.B, T, AC.H, dh)
    assert s_got.dtype == p_got.dtype == z_got.dtype == dtype
    ratios = AC.check(dtype, q, k, v, s_got, p_got, z_got, dh)
    line = AC.report(f"{_id(path)} {name}", ratios)
    if dtype == BF16:
        # the same element bound for a float32 torch softmax of the same stored scores, rounded to bf16: what rounding alone costs
        p_ref = AC.reference_pattern(s_got)
        p32 = torch.softmax(s_got.float(), dim=-1)
        p32 = torch.where(torch.isnan(p32), torch.zeros_like(p32), p32).to(BF16)
        line += f"  (fp32 torch softmax, rounded: pattern {AC.pattern_elementwise_ok(p32, p_ref)[1]:.3g})"
    print(line)
    assert AC.passes(dtype, ratios), line
    # the same pattern and the same z whichever taps are taken
    assert torch.equal(pat_z[pre + "hook_pattern"], p_got)
    assert torch.equal(pat_z[pre + "hook_z"], z_got) and torch.equal(only_z[pre + "hook_z"], z_got)


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) head-to-XCD assignment: recompute from the q, k, v the same run cached (test_dino_gpu.check_attention at any B, H)
# ---------------------------------------------------------------------------------------------------------------------------------
def recompute_bounds(cache, dtype, layer, B, H, T, d_head, tag=""):
    pre = f"blocks.{layer}.attn."
    q, k, v = (cache[pre + n].float() for n in ("hook_q", "hook_k", "hook_v"))
    assert q.shape == (B, T, H, d_head)
    s_ref = torch.einsum("bqhd,bkhd->bhqk", q, k) / (d_head ** 0.5)
    s_got = cache[pre + "hook_attn_scores"]
    assert s_got.shape == (B, H, T, T) and s_got.dtype == dtype
    close(s_got, s_ref, dtype, tag + "scores")
    p_ref = torch.softmax(s_got.float(), dim=-1)
    p_got = cache[pre + "hook_pattern"]
    assert p_got.shape == (B, H, T, T) and p_got.dtype == dtype
    close(p_got, p_ref, dtype, tag + "pattern", absolute=True)
    z_got = cache[pre + "hook_z"]
    assert z_got.shape == (B, T, H, d_head) and z_got.dtype == dtype
    z_ref = torch.einsum("bhqk,bkhd->bqhd", p_got.float(), v)
    close(z_got, z_ref, dtype, tag + "z")
    # per (image, head): a head computed from another head's rows passes a whole-tensor bound only by luck, not this one
    for b in range(B):
        for h in range(H):
            close(z_got[b, :, h], z_ref[b, :, h], dtype, f"{tag}z of image {b} head {h}")
    return p_ref


def check_attention(model, x, dtype, d_head, B, H, T):
    pre = "blocks.0.attn."
    with torch.no_grad():
        _, cache = model.run_with_cache(x)
        assert model.last_run_native, model.native_fallback_reason
        _, only_z = model.run_with_cache(x, names_filter=pre + "hook_z")                                               # no taps at all
        assert model.last_run_native
        _, pat_z = model.run_with_cache(x, names_filter=lambda n: n.endswith(("attn.hook_pattern", "attn.hook_z")))  # no score tap
        assert model.last_run_native
    p_ref = recompute_bounds(cache, dtype, 0, B, H, T, d_head)
    close(pat_z[pre + "hook_pattern"], p_ref, dtype, "pattern (no score tap)", absolute=True)
    assert torch.equal(only_z[pre + "hook_z"], cache[pre + "hook_z"])
    assert torch.equal(pat_z[pre + "hook_z"], cache[pre + "hook_z"])
    assert torch.equal(pat_z[pre + "hook_pattern"], cache[pre + "hook_pattern"])


@DTYPES
def test_nine_heads_of_80_one_whole_round_of_eight_plus_a_remainder(dtype):
    model = _build(dtype, 240, 3, 80, 128, 4, 32, 9)
    assert model.n_tokens == 65
    x = torch.randn(3, 3, 32, 32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(9)).to(dtype)
    check_attention(model, x, dtype, 80, 3, 3, 65)


def test_one_layer_of_vit_h14_geometry_bf16():
    model = _build(BF16, 1280, 16, 80, 5120, 14, 224, 14, n_classes=1024)
    assert model.n_tokens == 257
    x = torch.randn(2, 3, 224, 224, device="cuda", generator=torch.Generator(device="cuda").manual_seed(14)).to(BF16)
    check_attention(model, x, BF16, 80, 2, 16, 257)


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) whole model against the reference
# ---------------------------------------------------------------------------------------------------------------------------------
def _images(dtype, seed=1):
    return torch.from_numpy(synth_images(ARCHS["tiny-wide"], WIDE_BATCH, seed)).cuda().to(dtype)


def held(dtype, got, want, want32, tag):
    """test_native_vit_gpu's rule.  fp32: rel_fro < FP32_TOL against the PyTorch path; bf16: the error against the fp32 run is at most
    INTRA_BLOCK_RATIO times the PyTorch bf16 path's own."""
    a, b = got.float().cpu().numpy(), want.float().cpu().numpy()
    assert a.shape == b.shape, tag
    if dtype == F32:
        assert rel_fro(got.cpu(), want.cpu()) < FP32_TOL, tag
        return
    b32 = want32.float().cpu()
    budget, err = rel_fro(want.cpu(), b32), rel_fro(got.cpu(), b32)
    if budget == 0.0:
        assert np.array_equal(a, b), tag
    else:
        assert err <= INTRA_BLOCK_RATIO * budget, (tag, err, budget)


def test_wide_tiny_fp32_vs_reference_golden_tensors():
    G = np.load(os.path.join(GOLDEN, "vit_tiny_wide.npz"))
    model = wide_tiny_model(F32, "cuda").use_native(True)
    with torch.no_grad():
        out, cache = model.run_with_cache(_images(F32))
    assert model.last_run_native, model.native_fallback_reason
    keys = [str(k) for k in G["__keys__"]]
    assert list(cache.keys()) == keys
    for k in keys:
        assert cache[k].shape == G[k].shape and cache[k].dtype == F32, k
        assert rel_fro(cache[k].cpu(), torch.from_numpy(G[k])) < FP32_TOL, k
    assert rel_fro(out.cpu(), torch.from_numpy(G["__out__"])) < FP32_TOL
    for layer in range(2):
        recompute_bounds(cache, F32, layer, WIDE_BATCH, 2, 17, 80, f"layer {layer} ")


def test_wide_tiny_bf16_held_to_the_pytorch_bf16_paths_own_error():
    model = wide_tiny_model(BF16, "cuda").use_native(True)
    ref, ref32 = _pytorch_twin(model), wide_tiny_model(F32, "cuda").use_native(False)
    x = _images(BF16)
    with torch.no_grad():
        out, cache = model.run_with_cache(x)
        assert model.last_run_native, model.native_fallback_reason
        w_out, w_cache = ref.run_with_cache(x)
        assert not ref.last_run_native
        f_out, f_cache = ref32.run_with_cache(x.float())
    assert list(cache.keys()) == list(w_cache.keys()) == list(f_cache.keys())
    for k in w_cache.keys():
        assert cache[k].dtype == w_cache[k].dtype, k
        held(BF16, cache[k], w_cache[k], f_cache[k], k)
    held(BF16, out, w_out, f_out, "out")
    for layer in range(2):
        recompute_bounds(cache, BF16, layer, WIDE_BATCH, 2, 17, 80, f"layer {layer} ")


# ---------------------------------------------------------------------------------------------------------------------------------
# (d) hooks: the resumed attention core at d_head 80 (T = 17)
# ---------------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_hooked_scores_with_a_nan_row_and_an_all_minus_inf_row(dtype):
    model = wide_tiny_model(dtype, "cuda").use_native(True)
    x = _images(dtype)
    pre = "blocks.0.attn."

    def edit(t, hook=None):
        t = t.clone()
        t[0, 1, 5, 9] = float("nan")
        t[1, 0, 16, :] = float("-inf")
        return t

    with torch.no_grad():
        _, plain = model.run_with_cache(x, names_filter=lambda n: n in (pre + "hook_attn_scores", pre + "hook_v"))
        _, cache = model.run_with_cache(x, fwd_hooks=[(pre + "hook_attn_scores", edit)])
    assert model.last_run_native and not model.native_fallback_reason, model.native_fallback_reason
    p_got = cache[pre + "hook_pattern"]
    assert p_got.shape == (WIDE_BATCH, 2, 17, 17) and p_got.dtype == dtype
    assert float(p_got[0, 1, 5].abs().max()) == 0.0 and float(p_got[1, 0, 16].abs().max()) == 0.0
    p_ref = torch.softmax(edit(plain[pre + "hook_attn_scores"]).float(), dim=-1)
    p_ref = torch.where(torch.isnan(p_ref), torch.zeros_like(p_ref), p_ref)
    assert float(p_ref[0, 1, 5].abs().max()) == 0.0 and float(p_ref[1, 0, 16].abs().max()) == 0.0
    close(p_got, p_ref, dtype, "pattern behind the hook", absolute=True)
    z_got = cache[pre + "hook_z"]
    assert z_got.shape == (WIDE_BATCH, 17, 2, 80)
    z_ref = torch.einsum("bhqk,bkhd->bqhd", p_got.float(), plain[pre + "hook_v"].float())
    close(z_got, z_ref, dtype, "z behind the hook")
    close(z_got[..., 64:], z_ref[..., 64:], dtype, "z behind the hook, d >= 64 (the second round of lanes)")
    assert float(z_got[0, 5, 1].abs().max()) == 0.0 and float(z_got[1, 16, 0].abs().max()) == 0.0
    # block 1 went on from there on the plan: its own attention is consistent with its own q, k, v
    recompute_bounds(cache, dtype, 1, WIDE_BATCH, 2, 17, 80, "layer 1 ")


@DTYPES
def test_hooked_pattern_with_one_key_column_zeroed(dtype):
    model = wide_tiny_model(dtype, "cuda").use_native(True)
    x = _images(dtype)
    pre = "blocks.0.attn."

    def edit(t, hook=None):
        t = t.clone()
        t[..., 3] = 0
        return t

    with torch.no_grad():
        _, plain = model.run_with_cache(x, names_filter=lambda n: n in (pre + "hook_pattern", pre + "hook_v"))
        _, cache = model.run_with_cache(x, fwd_hooks=[(pre + "hook_pattern", edit)])
    assert model.last_run_native and not model.native_fallback_reason, model.native_fallback_reason
    z_got = cache[pre + "hook_z"]
    z_ref = torch.einsum("bhqk,bkhd->bqhd", edit(plain[pre + "hook_pattern"]).float(), plain[pre + "hook_v"].float())
    close(z_got, z_ref, dtype, "z behind the pattern hook")
    close(z_got[..., 64:], z_ref[..., 64:], dtype, "z behind the pattern hook, d >= 64")


@DTYPES
def test_head_ablation_through_hook_z(dtype):
    model = wide_tiny_model(dtype, "cuda").use_native(True)
    ref = _pytorch_twin(model)
    ref32 = wide_tiny_model(F32, "cuda").use_native(False) if dtype == BF16 else None
    x = _images(dtype)

    def kill_head_1(t, hook=None):
        t[:, :, 1] = 0.0

    hooks = [("blocks.0.attn.hook_z", kill_head_1)]
    with torch.no_grad():
        out, cache = model.run_with_cache(x, fwd_hooks=hooks)
        assert model.last_run_native and not model.native_fallback_reason, model.native_fallback_reason
        w_out, w_cache = ref.run_with_cache(x, fwd_hooks=hooks)
        f_out, f_cache = ref32.run_with_cache(x.float(), fwd_hooks=hooks) if ref32 is not None else (None, None)
    assert float(cache["blocks.0.attn.hook_z"][:, :, 1].abs().max()) == 0.0
    assert float(cache["blocks.0.attn.hook_z"][:, :, 0].abs().max()) > 0.0
    assert list(cache.keys()) == list(w_cache.keys())
    for k in w_cache.keys():
        held(dtype, cache[k], w_cache[k], f_cache[k] if f_cache is not None else None, k)
    held(dtype, out, w_out, f_out, "out")


# ---------------------------------------------------------------------------------------------------------------------------------
# (e) the derived attn.hook_result entry
# ---------------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_use_attn_result_entry_equals_the_pytorch_paths(dtype):
    model = wide_tiny_model(dtype, "cuda")
    model.set_use_attn_result(True)
    model.use_native(True)
    ref = _pytorch_twin(model)
    ref32 = None
    if dtype == BF16:
        ref32 = wide_tiny_model(F32, "cuda")
        ref32.set_use_attn_result(True)
        ref32.use_native(False)
    x = _images(dtype)
    with torch.no_grad():
        out, cache = model.run_with_cache(x)
        assert model.last_run_native and not model.native_fallback_reason, model.native_fallback_reason
        w_out, w_cache = ref.run_with_cache(x)
        f_out, f_cache = ref32.run_with_cache(x.float()) if ref32 is not None else (None, None)
    assert list(cache.keys()) == list(w_cache.keys())
    for layer in range(2):
        k = f"blocks.{layer}.attn.hook_result"
        assert cache[k].shape == (WIDE_BATCH, 17, 2, 160) and cache[k].dtype == dtype
        held(dtype, cache[k], w_cache[k], f_cache[k] if f_cache is not None else None, k)
    held(dtype, out, w_out, f_out, "out")
