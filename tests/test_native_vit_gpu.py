"""GPU parity tests of the native run_with_cache path (through the C ABI) against the numpy oracle
and the reference-generated golden fixtures.  Run with ``-m gpu`` on an MI355X.

Tolerances (stated per north_star / SURVEY.md section 7 hard part 1):
  * fp32 mode: rel-Frobenius <= 1e-4 per cache tensor vs the fp32 oracle (measured ~2e-6)
  * bf16 mode: error vs the fp32 oracle <= 1.0 x the reference's OWN bf16-vs-fp32 error for the same key on the same
    images (tests/golden/vit_*_bf16_budget*.json, produced by running the reference with cfg.dtype=bf16; one documented
    exception class, see bf16_limit); a 1e-4 bound is unattainable for any bf16 pipeline, the reference's included
  * hook names / order / shapes / dtypes: exact
"""
import json
import os

import numpy as np
import pytest
import torch

from oracle.vit_oracle import fingerprint, hook_names_in_order, vit_forward
from vit_prisma_amd import ActivationCache, HookedViT, HookedViTConfig, _native
from vit_prisma_amd.synth import ARCHS, synth_images, synth_vit_state

from _attention_cases import pattern_elementwise_ok
from conftest import GOLDEN, rel_fro

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4

# bf16 bar (hard part 1(ii)): error vs the fp32 oracle <= 1.0 x the error the REFERENCE's own bf16 run
# has for the same key on the same images.  Measured at bs = 512 (profiles/r02_parity_ratios.json): 211 of 214 keys at
# 0.94-1.000 (the embedding / ln_pre / block-0 keys are BIT-identical to the reference's bf16 tensors, ratio 1.000000).
# One documented exception class: ``*.hook_scale`` -- fp32 per-token scalars sqrt(mean(x^2) + eps) of a bf16 residual
# stream (budget 2e-4 .. 5e-4).  Their error is the rounding noise of that stream, which is independent of (and as large
# as) the reference's, so the per-key ratio scatters around 1 and the scatter shrinks with the number of rows averaged:
# measured <= 1.022 over the 16 checked images of the bs = 512 bench batch (held to 1.05 x there), <= 1.13 on the 4-image
# fixture (held to 1.15 x; profiles/r02_parity_ratios.json).
# BF16_SLACK: "1.0 x" is asserted up to 1e-4 relative: the early keys reproduce the reference's bf16 tensors up to a
# handful of differently rounded elements (measured ratios 1.000000 .. 1.000004), and the budget itself was computed with
# torch's norm, the test with numpy's.
BF16_SLACK = 1.0 + 1e-4
SCALE_SLACK_SMALL, SCALE_SLACK_BENCH = 1.15, 1.05
# intra-block hooks on the tiny models in bf16: HIP error vs the fp32 run, as a multiple of the PyTorch bf16 path's own error
INTRA_BLOCK_RATIO = 1.5


def bf16_limit(key: str, budget_rel_fro: float, scale_slack: float = SCALE_SLACK_SMALL, ln_taps: bool = False) -> float:
    """ln_taps (the massive-activation state only): the exception class of ``*.hook_scale`` extended to ``*.hook_normalized`` -- the other fp32
    tap of a LayerNorm over the bf16 residual stream.  With outlier channels at |x| ~ 100 (bf16 ulp 0.5) the tap's error IS the rounding
    noise of those few channels, independent of (and as large as) the reference's own: the per-key ratio scatters around 1 exactly as
    hook_scale's does (measured 1.005 on blocks.4.ln1.hook_normalized of the 4-image fixture, every other key <= 1.0)."""
    slack = key.endswith(".hook_scale") or (ln_taps and key.endswith(".hook_normalized"))
    return budget_rel_fro * (scale_slack if slack else 1.0) * BF16_SLACK


def build(arch_name, dtype, outliers=False):
    arch = ARCHS[arch_name]
    model = HookedViT(HookedViTConfig(**arch, dtype=dtype, device="cuda"))
    sd = synth_vit_state(arch, 0, outliers=outliers)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return model.to(dtype).cuda().eval().use_native(True), arch, sd


def run(model, imgs, dtype, **kw):
    with torch.no_grad():
        out, cache = model.run_with_cache(torch.from_numpy(imgs).cuda().to(dtype), **kw)
    torch.cuda.synchronize()
    assert model.last_run_native, model.native_fallback_reason
    return out, cache


def test_native_library_is_loaded():
    lib = _native.lib()
    assert lib.pv_abi_version() == _native.ABI_VERSION
    with open("/proc/self/maps") as f:
        assert "libpvnative.so" in f.read()
    # the prebuilt library travels next to the sources: it must have been built from exactly these files
    assert _native.build_id() == _native.source_id(), "libpvnative.so is stale: run python -m vit_prisma_amd.build"


@pytest.mark.parametrize("arch_name", ["tiny", "tiny-ragged"])
@pytest.mark.parametrize("stop", [None, 1, 0, -1])
def test_fp32_small_vs_oracle(arch_name, stop):
    model, arch, sd = build(arch_name, torch.float32)
    imgs = synth_images(arch, 3, 1)
    o_ref, c_ref = vit_forward(sd, arch, imgs, stop_at_layer=stop)
    out, cache = run(model, imgs, torch.float32, stop_at_layer=stop)
    assert list(cache.keys()) == list(c_ref.keys())
    for k, ref in c_ref.items():
        assert tuple(cache[k].shape) == ref.shape and cache[k].dtype == torch.float32, k
        assert rel_fro(cache[k].cpu().numpy(), ref) < FP32_TOL, k
    assert rel_fro(out.cpu().numpy(), o_ref) < FP32_TOL


@pytest.mark.parametrize("fname,arch_name,bs", [("vit_tiny_full.npz", "tiny", 3), ("vit_tiny_ragged_full.npz", "tiny-ragged", 2)])
def test_fp32_small_vs_reference_golden_tensors(fname, arch_name, bs):
    g = np.load(os.path.join(GOLDEN, fname))
    model, arch, _ = build(arch_name, torch.float32)
    out, cache = run(model, synth_images(arch, bs, 1), torch.float32)
    keys = [str(k) for k in g["__keys__"]]
    assert list(cache.keys()) == keys
    for k in keys:
        assert rel_fro(cache[k].cpu().numpy(), g[k]) < FP32_TOL, k
    assert rel_fro(out.cpu().numpy(), g["__out__"]) < FP32_TOL


def test_fp32_b32_bs16_all_hooks_vs_oracle_and_golden():
    """BASELINE config 1: 16 random 224x224 images, all hook names, keys/shapes asserted."""
    with open(os.path.join(GOLDEN, "vit_b32_fp32_bs16.json")) as f:
        G = json.load(f)["all"]
    model, arch, sd = build("clip-vit-b32", torch.float32)
    imgs = synth_images(arch, 16, 1)
    o_ref, c_ref = vit_forward(sd, arch, imgs)
    out, cache = run(model, imgs, torch.float32)
    assert isinstance(cache, ActivationCache)
    assert list(cache.keys()) == G["keys"] == list(c_ref.keys()) and len(cache) == 214
    for k, ref in c_ref.items():
        got = cache[k].cpu().numpy()
        assert list(got.shape) == G["cache"][k]["shape"], k
        assert rel_fro(got, ref) < FP32_TOL, k
        fp = fingerprint(got)                       # the reference's own run, fingerprinted
        assert abs(fp["l2"] - G["cache"][k]["l2"]) <= FP32_TOL * G["cache"][k]["l2"], k
        vw = np.array(G["cache"][k]["vals"])
        assert np.max(np.abs(np.array(fp["vals"]) - vw)) <= 1e-3 * max(np.max(np.abs(vw)), G["cache"][k]["l2"] / np.sqrt(got.size)), k
    assert rel_fro(out.cpu().numpy(), o_ref) < FP32_TOL
    # aliases of the reference (same storage there, same tensor here)
    assert cache["blocks.3.hook_resid_post"].data_ptr() == cache["blocks.4.hook_resid_pre"].data_ptr()
    assert cache["hook_ln_pre"].data_ptr() == cache["blocks.0.hook_resid_pre"].data_ptr()
    assert cache["hook_pos_embed"].stride(0) == 0


@pytest.mark.parametrize("tile", [None, "5", "4", "0"])
def test_bf16_b32_within_reference_bf16_budget(tile, tuning):
    """tile: the GEMM kernel the library would pick by itself at this size (128 x 128, 3 workgroups per CU), then the
    large-batch kernels forced onto the same small problem (pv_debug_set_tuning gemm_tile: 320 x 256 / 256 x 256 tile, one 8-wave
    workgroup per CU, compile-time epilogues) -- every variant has to meet the same budget."""
    if tile is not None:
        tuning("gemm_tile", int(tile))
    with open(os.path.join(GOLDEN, "vit_b32_bf16_budget.json")) as f:
        budget = json.load(f)["budget"]
    model, arch, sd = build("clip-vit-b32", torch.bfloat16)
    imgs = synth_images(arch, 4, 1)
    o_ref, c_ref = vit_forward(sd, arch, imgs)
    out, cache = run(model, imgs, torch.bfloat16)
    assert list(cache.keys()) == list(c_ref.keys())
    n32 = 0
    for k, ref in c_ref.items():
        # dtype contract: ln*.hook_scale / hook_normalized fp32, everything else bf16 (52 + 162 keys)
        assert str(cache[k].dtype) == budget[k]["dtype_bf16_run"], k
        n32 += cache[k].dtype == torch.float32
        err = rel_fro(cache[k].float().cpu().numpy(), ref)
        assert err <= bf16_limit(k, budget[k]["rel_fro"]), (k, err, budget[k]["rel_fro"])
    assert n32 == 52
    assert rel_fro(out.float().cpu().numpy(), o_ref) <= budget["__out__"]["rel_fro"] * BF16_SLACK


def test_fp32_b32_outliers_vs_oracle_and_golden():
    """VERDICT r5 item 4a, fp32 form: all 214 keys on the massive-activation state (synth_vit_state(outliers=True): residual channels
    at |x| ~ 100 beside an rms of ~1.2) against the oracle at 1e-4 and against the REFERENCE's own fp32 run, fingerprinted
    (tests/golden/vit_b32_outliers_bf16_budget.json)."""
    with open(os.path.join(GOLDEN, "vit_b32_outliers_bf16_budget.json")) as f:
        G = json.load(f)
    model, arch, sd = build("clip-vit-b32", torch.float32, outliers=True)
    imgs = synth_images(arch, G["batch"], G["seed"])
    o_ref, c_ref = vit_forward(sd, arch, imgs)
    out, cache = run(model, imgs, torch.float32)
    want = G["fp32"]
    assert list(cache.keys()) == want["keys"] == list(c_ref.keys()) and len(cache) == 214
    for k, ref in c_ref.items():
        got = cache[k].cpu().numpy()
        assert rel_fro(got, ref) < FP32_TOL, k
        fp = fingerprint(got)
        assert abs(fp["l2"] - want["cache"][k]["l2"]) <= FP32_TOL * want["cache"][k]["l2"], k
        vw = np.array(want["cache"][k]["vals"])
        assert np.max(np.abs(np.array(fp["vals"]) - vw)) <= 1e-3 * max(np.max(np.abs(vw)), want["cache"][k]["l2"] / np.sqrt(got.size)), k
    assert rel_fro(out.cpu().numpy(), o_ref) < FP32_TOL


def test_bf16_b32_outliers_within_reference_bf16_budget():
    """VERDICT r5 item 4a, bf16 form -- the bar "error vs the fp32 oracle <= 1.0 x the reference's OWN bf16 error, key by key" where bf16
    is actually stressed: on the massive-activation state (ulp(100) = 0.5 in bf16 beside values of ~1), all 214 keys on the 4-image
    batch, then images 0-7 / 504-511 of the bs = 512 bench batch with the kernels the library picks at that size."""
    with open(os.path.join(GOLDEN, "vit_b32_outliers_bf16_budget.json")) as f:
        G = json.load(f)
    model, arch, sd = build("clip-vit-b32", torch.bfloat16, outliers=True)
    imgs = synth_images(arch, G["batch"], G["seed"])
    o_ref, c_ref = vit_forward(sd, arch, imgs)
    out, cache = run(model, imgs, torch.bfloat16)
    assert list(cache.keys()) == list(c_ref.keys()) and len(cache) == 214
    _held_to_budget(cache, c_ref, G["budget"], slice(None), "outliers bs=4", SCALE_SLACK_SMALL, ln_taps=True)
    assert rel_fro(out.float().cpu().numpy(), o_ref) <= G["budget"]["__out__"]["rel_fro"] * BF16_SLACK
    del cache
    S = G["sub512"]
    sub = S["images"]
    big = synth_images(arch, S["batch"], S["seed"])
    o_ref, c_ref = vit_forward(sd, arch, big[sub])
    out, cache = run(model, big, torch.bfloat16)
    assert len(cache) == 214
    _held_to_budget(cache, c_ref, S["budget"], sub, "outliers bs=512", ln_taps=True)
    assert rel_fro(out[sub].float().cpu().numpy(), o_ref) <= S["budget"]["__out__"]["rel_fro"] * BF16_SLACK


def test_filters_stop_remove_batch_and_cpu_device():
    model, arch, sd = build("clip-vit-b32", torch.float32)
    imgs = synth_images(arch, 4, 1)
    # the harvest form of VisionActivationsStore.get_activations
    o_ref, c_ref = vit_forward(sd, arch, imgs, stop_at_layer=7, names_filter=["blocks.6.hook_resid_post"])
    out, cache = run(model, imgs, torch.float32, stop_at_layer=7, names_filter=["blocks.6.hook_resid_post"])
    assert list(cache.keys()) == ["blocks.6.hook_resid_post"]
    assert rel_fro(out.cpu().numpy(), o_ref) < FP32_TOL and torch.equal(out, cache["blocks.6.hook_resid_post"])
    # callable filter, str filter + remove_batch_dim, device="cpu" (pinned mirror, one D2H copy)
    flt = lambda n: n.endswith("hook_pattern") or n == "hook_embed"  # noqa: E731
    _, c_ref = vit_forward(sd, arch, imgs[:2], names_filter=flt)
    _, cache = run(model, imgs[:2], torch.float32, names_filter=flt, device="cpu")
    assert list(cache.keys()) == list(c_ref.keys())
    for k, ref in c_ref.items():
        assert cache[k].device.type == "cpu" and rel_fro(cache[k].numpy(), ref) < FP32_TOL, k
    _, c_ref = vit_forward(sd, arch, imgs[:1], names_filter="blocks.3.attn.hook_z")
    _, cache = run(model, imgs[:1], torch.float32, names_filter="blocks.3.attn.hook_z", remove_batch_dim=True)
    assert cache["z", 3].shape == (50, 12, 64) and not cache.has_batch_dim
    assert rel_fro(cache["z", 3].cpu().numpy(), c_ref["blocks.3.attn.hook_z"][0]) < FP32_TOL
    # return_cache_object=False gives the plain dict
    with torch.no_grad():
        _, d = model.run_with_cache(torch.from_numpy(imgs[:1]).cuda(), return_cache_object=False, names_filter="hook_embed")
    assert isinstance(d, dict) and list(d) == ["hook_embed"]


def test_cache_lifetime_ring_never_overwrites_live_entries():
    model, arch, _ = build("tiny", torch.float32)
    x1 = torch.from_numpy(synth_images(arch, 2, 1)).cuda()
    x2 = torch.from_numpy(synth_images(arch, 2, 2)).cuda()
    with torch.no_grad():
        _, c1 = model.run_with_cache(x1)
        keep = {k: v.clone() for k, v in c1.items()}
        for _ in range(6):                          # more calls than ring slabs while c1 is alive
            _, c2 = model.run_with_cache(x2)
        torch.cuda.synchronize()
        for k in keep:
            assert torch.equal(c1[k], keep[k]), k   # c1's slab was never handed out again
        del c1, c2
        n_alloc = model._native.arena.n_alloc
        for _ in range(4):
            _, c3 = model.run_with_cache(x2)
            del c3
        assert model._native.arena.n_alloc == n_alloc   # steady state: slabs recycled, no allocation


def test_native_equals_pytorch_hook_path_and_fallback_dispatch():
    model, arch, _ = build("tiny", torch.float32)
    x = torch.from_numpy(synth_images(arch, 2, 1)).cuda()
    with torch.no_grad():
        out_n, c_n = model.run_with_cache(x)
        assert model.last_run_native
        model.use_native(False)
        out_t, c_t = model.run_with_cache(x)
        assert not model.last_run_native
        assert list(c_n.keys()) == list(c_t.keys())
        for k in c_t.keys():
            assert c_n[k].shape == c_t[k].shape and c_n[k].dtype == c_t[k].dtype, k
            assert rel_fro(c_n[k].cpu().numpy(), c_t[k].cpu().numpy()) < FP32_TOL, k
        # a mutating user hook on a residual-stream point (or on q / k / v / z / mlp post) splits the native plan; anywhere
        # else it must run as a Python callback inside the PyTorch forward: auto mode falls back, force mode raises
        model.use_native(None)
        zero = lambda t, hook: torch.zeros_like(t)  # noqa: E731
        _, c_h = model.run_with_cache(x, fwd_hooks=[("blocks.0.hook_attn_out", zero)])
        assert model.last_run_native and float(c_h["blocks.0.hook_attn_out"].abs().max()) == 0.0
        assert torch.equal(c_h["blocks.0.hook_resid_mid"], c_h["blocks.0.hook_resid_pre"])
        _, c_h = model.run_with_cache(x, fwd_hooks=[("blocks.0.attn.hook_z", zero)])           # inside the block: split there too
        assert model.last_run_native and float(c_h["blocks.0.attn.hook_z"].abs().max()) == 0.0
        _, c_h = model.run_with_cache(x, fwd_hooks=[("blocks.0.attn.hook_pattern", zero)])           # ... and at the pattern
        assert model.last_run_native and float(c_h["blocks.0.attn.hook_pattern"].abs().max()) == 0.0
        assert float(c_h["blocks.0.attn.hook_z"].abs().max()) == 0.0
        _, c_h = model.run_with_cache(x, fwd_hooks=[("blocks.0.mlp.hook_pre", zero)])                # ... at the MLP pre-activation
        assert model.last_run_native and float(c_h["blocks.0.mlp.hook_pre"].abs().max()) == 0.0
        _, c_h = model.run_with_cache(x, fwd_hooks=[("hook_embed", zero)])     # embedding stage on the modules, blocks on the plan
        assert model.last_run_native and float(c_h["hook_embed"].abs().max()) == 0.0
        # a plain nn.Module hook is invisible to the plan: auto mode takes the PyTorch path, force mode raises
        seen = []
        handle = model.blocks[0].register_forward_hook(lambda m, i, o: seen.append(1))
        _, c_h = model.run_with_cache(x)
        assert not model.last_run_native and seen and "nn.Module hooks" in model.native_fallback_reason
        model.use_native(True)
        with pytest.raises(_native.NativeError):
            model.run_with_cache(x)
        handle.remove()
    # weight edits are picked up (version counter) -> output changes
    model.use_native(True)
    with torch.no_grad():
        model.blocks[0].mlp.W_out.mul_(0.0)
        out2, _ = model.run_with_cache(x)
    assert not torch.allclose(out2, out_n)


def test_l14_336_pattern_hooks_fp32():
    with open(os.path.join(GOLDEN, "vit_l14_fp32_bs1.json")) as f:
        G = json.load(f)
    model, arch, sd = build("clip-vit-l14-336", torch.float32)
    imgs = synth_images(arch, 1, 1)
    want = G["sel"]["keys"]
    out, cache = run(model, imgs, torch.float32, names_filter=want)
    assert list(cache.keys()) == want
    for k in want:
        fp, gw = fingerprint(cache[k].cpu().numpy()), G["sel"]["cache"][k]
        assert fp["shape"] == gw["shape"] == [1, 16, 577, 577]
        assert abs(fp["l2"] - gw["l2"]) <= FP32_TOL * gw["l2"], k
        assert np.max(np.abs(np.array(fp["vals"]) - np.array(gw["vals"]))) <= 1e-3 * max(np.max(np.abs(gw["vals"])), 1e-3), k
    assert abs(fingerprint(out.cpu().numpy())["l2"] - G["sel"]["out"]["l2"]) < 1e-4
    # all-hooks key/shape inventory (418 keys) at bs=1
    _, call = run(model, imgs, torch.float32)
    assert list(call.keys()) == G["all_keys"] == hook_names_in_order(arch)
    for k, shp in G["all_shapes"].items():
        assert list(call[k].shape) == shp, k
    # softmax rows sum to one at full size (size-independent property)
    s = call["blocks.23.attn.hook_pattern"].sum(-1)
    assert float((s - 1).abs().max()) < 1e-5


def test_bf16_full_size_properties_bs512():
    """BASELINE config 2 shape (bs=512 bf16, all hooks): properties that need no oracle."""
    model, arch, _ = build("clip-vit-b32", torch.bfloat16, outliers=True)
    x = torch.randn(512, 3, 224, 224, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0)).bfloat16()
    with torch.no_grad():
        out, cache = model.run_with_cache(x)
    assert len(cache) == 214 and out.shape == (512, 512)
    assert torch.isfinite(out.float()).all()
    assert float((out.float().norm(dim=-1) - 1).abs().max()) < 1e-2            # F.normalize
    for l in (0, 5, 11):
        p = cache["pattern", l].float()
        assert p.shape == (512, 12, 50, 50) and float((p.sum(-1) - 1).abs().max()) < 2e-2
        # resid_mid == resid_pre + attn_out up to one bf16 rounding
        lhs = cache["resid_mid", l].float()
        rhs = cache["resid_pre", l].float() + cache["attn_out", l].float()
        assert float(((lhs - rhs).abs() / (rhs.abs() + 1.0)).max()) < 1e-2
        # post == gelu(pre) applied to the stored bf16 pre
        pre = cache["pre", l].float()
        assert float((cache["post", l].float() - torch.nn.functional.gelu(pre)).abs().max()) < 5e-2
    # batch independence: image 17 alone gives the same row (bitwise: no cross-image reduction anywhere)
    with torch.no_grad():
        out1, _ = model.run_with_cache(x[17:18], names_filter="hook_embed")
    assert torch.equal(out1[0], out[17])


@pytest.mark.parametrize("arch_name,bs", [("clip-vit-b32", 5), ("tiny-ragged", 3), ("clip-vit-l14-336", 1)])
def test_bf16_attention_core_against_fp32_recompute_of_its_own_inputs(arch_name, bs):
    """The attention kernels in isolation: scores / pattern / z recomputed in fp32 torch from the q, k, v the
    same run cached (so every input is bit-identical), against the bf16 taps.  Token counts 50 and 10 (even): the
    one-head-per-wave kernel; 577 (L/14@336): the query-block kernel with its bf16 score block in LDS.
    Bound = one bf16 rounding of each stage (2^-8 relative), attention.py:246-281."""
    model, arch, sd = build(arch_name, torch.bfloat16)
    out, cache = run(model, synth_images(arch, bs, 3), torch.bfloat16)
    for layer in range(arch["n_layers"]):
        pre = f"blocks.{layer}.attn."
        q, k, v = (cache[pre + n].float() for n in ("hook_q", "hook_k", "hook_v"))          # [B, T, H, dh]
        scale = float(arch["d_head"]) ** 0.5
        s_ref = torch.einsum("bqhd,bkhd->bhqk", q, k) / scale
        s_got = cache[pre + "hook_attn_scores"].float()
        assert s_got.shape == s_ref.shape
        assert float((s_got - s_ref).abs().max()) <= 2 ** -8 * float(s_ref.abs().max()) + 1e-6, layer
        # softmax of the STORED (bf16) scores, as the reference does
        p_ref = torch.softmax(s_got, dim=-1)
        p_got = cache[pre + "hook_pattern"].float()
        assert float((p_got - p_ref).abs().max()) <= 2 ** -8, layer
        # per element, relative: 2^-8 p + 1e-30 (tests/_attention_cases.py) -- the absolute bound alone passes an all-zero pattern at T = 577
        assert pattern_elementwise_ok(p_got, p_ref)[0], (layer, pattern_elementwise_ok(p_got, p_ref)[1])
        assert torch.allclose(p_got.sum(-1), torch.ones_like(p_got.sum(-1)), atol=2e-2)
        z_ref = torch.einsum("bhqk,bkhd->bqhd", p_got, v)
        z_got = cache[pre + "hook_z"].float()
        assert float((z_got - z_ref).abs().max()) <= 2 ** -8 * float(z_ref.abs().max()) + 1e-6, layer


def _pytorch_twin(model):
    """Same weights, PyTorch hook path only."""
    import copy
    twin = copy.deepcopy(model)
    twin._native = None
    return twin.use_native(False)


@pytest.mark.parametrize("arch_name", ["tiny", "tiny-ragged"])
def test_boundary_hooks_run_on_the_split_native_plan(arch_name):
    """replacement / ablation hooks on a block's residual-stream points (hook_resid_pre, hook_attn_out,
    hook_resid_mid, hook_mlp_out, hook_resid_post) keep the HIP path: the plan is split at the hook -- at a block
    boundary or after the attention half -- Python sees the tensor, the rest resumes from what it returned; every
    result must equal the PyTorch hook path of the same model (hooked_root_module.py:176-210), cache included."""
    model, arch, sd = build(arch_name, torch.float32)
    ref = _pytorch_twin(model)
    x = torch.from_numpy(synth_images(arch, 3, 5)).cuda()
    nl = arch["n_layers"]

    def scale_shift(t, hook):
        return t * 0.5 + 1.0

    def zero_cls(t, hook):                # in-place edit, returns None
        t[:, 0] = 0.0

    cases = [
        [("blocks.0.hook_resid_post", scale_shift)],
        [(f"blocks.{nl - 1}.hook_resid_post", zero_cls)],
        [("blocks.1.hook_resid_pre", scale_shift), ("blocks.0.hook_resid_post", zero_cls)],
        [(lambda n: n.endswith("hook_resid_post"), scale_shift)],
        [("blocks.0.hook_mlp_out", scale_shift)],
        [("blocks.0.hook_attn_out", scale_shift)],
        [("blocks.1.hook_resid_mid", zero_cls), ("blocks.1.hook_attn_out", scale_shift)],
        [(lambda n: n.endswith(("hook_attn_out", "hook_resid_mid", "hook_mlp_out", "hook_resid_post")) or n == "blocks.1.hook_resid_pre", scale_shift)],
        [(f"blocks.{nl - 1}.hook_mlp_out", zero_cls), (f"blocks.{nl - 1}.hook_resid_post", scale_shift), ("blocks.1.hook_resid_pre", zero_cls)],
    ]
    with torch.no_grad():
        for hooks in cases:
            want = ref.run_with_hooks(x.clone(), fwd_hooks=hooks)
            got = model.run_with_hooks(x.clone(), fwd_hooks=hooks)
            assert model.last_run_native, model.native_fallback_reason
            assert rel_fro(got.cpu().numpy(), want.cpu().numpy()) < FP32_TOL
            assert all(len(hp.fwd_hooks) == 0 for hp in model.hook_dict.values())          # context cleaned up
            # with caching, with a filter and with stop_at_layer
            for kw in ({}, {"names_filter": lambda n: "resid" in n or n.endswith("hook_pattern")}, {"stop_at_layer": nl - 1}):
                w_out, w_cache = ref.run_with_cache(x.clone(), fwd_hooks=hooks, **kw)
                g_out, g_cache = model.run_with_cache(x.clone(), fwd_hooks=hooks, **kw)
                assert model.last_run_native, model.native_fallback_reason
                assert list(g_cache.keys()) == list(w_cache.keys())
                assert rel_fro(g_out.cpu().numpy(), w_out.cpu().numpy()) < FP32_TOL
                for k in w_cache.keys():
                    a, b = g_cache[k].float().cpu().numpy(), w_cache[k].float().cpu().numpy()
                    assert a.shape == b.shape and rel_fro(a, b) < FP32_TOL, (k, kw)
        # a hook on a point the forward never calls with its flag off (flag-gated, transformer_block.py:88-104, 125-129) cannot fire:
        # the run stays on the plan and equals the PyTorch path's; a backward hook is what the plan cannot serve -- PyTorch path in
        # "auto" mode, an error in "force" mode
        model.use_native(None)
        out = model.run_with_hooks(x, fwd_hooks=[("blocks.0.hook_mlp_in", scale_shift)])
        assert model.last_run_native
        assert rel_fro(out.cpu().numpy(), ref.run_with_hooks(x, fwd_hooks=[("blocks.0.hook_mlp_in", scale_shift)]).cpu().numpy()) < FP32_TOL
        ident = lambda t, hook: None  # noqa: E731
        model.run_with_hooks(x, bwd_hooks=[("blocks.0.hook_resid_post", ident)])
        assert not model.last_run_native and "cannot be split" in model.native_fallback_reason
        model.use_native(True)
        with pytest.raises(_native.NativeError):
            model.run_with_hooks(x, bwd_hooks=[("blocks.0.hook_resid_post", ident)])
        assert all(len(hp.fwd_hooks) == 0 for hp in model.hook_dict.values())


@pytest.mark.parametrize("arch_name,dtype", [("tiny", torch.float32), ("tiny-ragged", torch.float32), ("tiny", torch.bfloat16)])
def test_embedding_and_final_stage_hooks_keep_the_blocks_on_the_hip_plan(arch_name, dtype):
    """Mutating hooks on hook_embed / hook_pos_embed / hook_full_embed / ln_pre.* / hook_ln_pre / blocks.0.hook_resid_pre and on
    ln_final.* / hook_ln_final / hook_post_head_pre_normalize (base_vit.py:169-185, 192-217): the hooked stage runs on the model's own
    PyTorch modules, every block on the HIP plan -- resumed at block 0 from the residual stream the embedding stage left, stopped
    before ln_final -- and the result equals the PyTorch hook path (fp32: 1e-4; bf16: held to the PyTorch bf16 path's own error
    against the fp32 run, as for the hooks inside a block)."""
    model, arch, sd = build(arch_name, dtype)
    ref = _pytorch_twin(model)
    x = torch.from_numpy(synth_images(arch, 3, 5)).cuda().to(dtype)
    nl = arch["n_layers"]
    ref32 = x32 = None
    if dtype == torch.bfloat16:
        m32, _, _ = build(arch_name, torch.float32)
        ref32, x32 = _pytorch_twin(m32), x.float()

    def scale_shift(t, hook):
        return t * 0.5 + 1.0

    def half(t, hook):
        return t * 0.5

    def zero_cls(t, hook):
        t[:, 0] = 0.0

    def kill_head_1(t, hook):
        t[:, :, 1] = 0.0

    def freeze_scale(t, hook):
        return torch.full_like(t, 1.25)

    cases = [
        [("hook_embed", scale_shift)],
        [("hook_pos_embed", half), ("blocks.0.hook_resid_pre", zero_cls)],
        [("hook_full_embed", zero_cls)],
        [("ln_final.hook_normalized", half)],
        [("ln_final.hook_scale", freeze_scale)],
        [("hook_ln_final", scale_shift)],
        [("hook_post_head_pre_normalize", half)],
        [("hook_embed", half), ("blocks.1.attn.hook_z", kill_head_1), ("ln_final.hook_normalized", half)],
        [("hook_embed", zero_cls), ("blocks.0.ln1.hook_scale", freeze_scale), (f"blocks.{nl - 1}.hook_resid_post", half), ("ln_final.hook_scale", half)],
    ]
    if arch.get("layer_norm_pre"):
        cases += [[("ln_pre.hook_scale", freeze_scale)], [("ln_pre.hook_normalized", half), ("hook_ln_pre", scale_shift)],
                  [("hook_ln_pre", zero_cls), ("blocks.0.attn.hook_q", half), ("hook_post_head_pre_normalize", half)]]

    def held(a, b, b32, tag):
        if dtype == torch.float32:
            assert rel_fro(a, b) < FP32_TOL, tag
            return
        budget, err = rel_fro(b, b32), rel_fro(a, b32)
        if budget == 0.0:
            assert np.array_equal(a, b), tag
        else:
            assert err <= INTRA_BLOCK_RATIO * budget, (tag, err, budget)

    with torch.no_grad():
        for ci, hooks in enumerate(cases):
            n0 = model._native.n_forward if model._native is not None else 0
            want = ref.run_with_hooks(x.clone(), fwd_hooks=hooks)
            got = model.run_with_hooks(x.clone(), fwd_hooks=hooks)
            assert model.last_run_native, model.native_fallback_reason
            assert model._native.n_forward > n0                               # the blocks did run on the HIP plan
            w32 = ref32.run_with_hooks(x32.clone(), fwd_hooks=hooks).cpu().numpy() if ref32 is not None else None
            held(got.float().cpu().numpy(), want.float().cpu().numpy(), w32, (ci, "out"))
            assert all(len(hp.fwd_hooks) == 0 and len(hp._forward_hooks) == 0 for hp in model.hook_dict.values())
            for kw in ({}, {"names_filter": lambda n: not n.startswith("blocks.") or "resid" in n}, {"stop_at_layer": nl - 1}, {"stop_at_layer": 0}):
                w_out, w_cache = ref.run_with_cache(x.clone(), fwd_hooks=hooks, **kw)
                g_out, g_cache = model.run_with_cache(x.clone(), fwd_hooks=hooks, **kw)
                assert model.last_run_native, model.native_fallback_reason
                assert list(g_cache.keys()) == list(w_cache.keys())
                f_out = f_cache = None
                if ref32 is not None:
                    f_out, f_cache = ref32.run_with_cache(x32.clone(), fwd_hooks=hooks, **kw)
                    f_out = f_out.cpu().numpy()
                held(g_out.float().cpu().numpy(), w_out.float().cpu().numpy(), f_out, (ci, "out", sorted(kw)))
                for k in w_cache.keys():
                    a, b = g_cache[k].float().cpu().numpy(), w_cache[k].float().cpu().numpy()
                    assert a.shape == b.shape, (k, kw)
                    held(a, b, f_cache[k].float().cpu().numpy() if f_cache is not None else None, (ci, k, sorted(kw)))


@pytest.mark.parametrize("arch_name,dtype", [("tiny", torch.float32), ("tiny-ragged", torch.float32), ("tiny", torch.bfloat16)])
def test_hooks_inside_the_attention_half_and_the_mlp_run_on_the_split_native_plan(arch_name, dtype):
    """Head ablation (attn.hook_z), edits of q / k / v, of the attention scores and of the pattern, frozen / edited LayerNorms
    (ln1 / ln2 .hook_scale / .hook_normalized), edits of mlp.hook_pre and neuron ablation (mlp.hook_post) keep the HIP path: the
    plan is
    split INSIDE the block (pv_vit_forward_stage) -- the hook sees the stage's activation, the rest of the block resumes from
    what it returned, the residual stream it adds to is carried along.  Every result must equal the PyTorch hook path of the
    same model (prisma_tools/hook_point.py:44-45; models/layers/attention.py:135-152, 186-281; mlp.py:65-80), cache
    included; bf16: within the bf16 budget of the un-hooked comparison."""
    model, arch, sd = build(arch_name, dtype)
    ref = _pytorch_twin(model)
    x = torch.from_numpy(synth_images(arch, 3, 5)).cuda().to(dtype)
    nl = arch["n_layers"]

    def half(t, hook):
        return t * 0.5

    def kill_head_1(t, hook):             # in place, returns None: [B, T, H, dh]
        t[:, :, 1] = 0.0

    def kill_neurons(t, hook):            # [B, T, d_mlp]
        t[..., ::3] = 0.0

    def swap_heads(t, hook):
        return t.flip(2)

    def no_cls_attention(t, hook):        # pattern [B, H, T, T]: nobody attends to the CLS token; rows renormalised
        t = t.clone()
        t[..., 0] = 0.0
        return t / t.sum(-1, keepdim=True).clamp_min(1e-6)

    def mask_scores(t, hook):             # scores [B, H, T, T], in place: head 0 cannot see the last key
        t[:, 0, :, -1] = float("-inf")

    def nan_row(t, hook):                 # a NaN score poisons its row: the reference's where(isnan) zeroes the pattern row
        t[:, 1, 2, 3] = float("nan")

    def freeze_scale(t, hook):            # "frozen LayerNorm": the scale [B, T, 1] replaced by a constant
        return torch.full_like(t, 1.25)

    def shift_pre(t, hook):
        return t - 0.25

    cases = [
        [("blocks.0.ln1.hook_scale", freeze_scale)],
        [("blocks.1.ln2.hook_normalized", half), ("blocks.1.mlp.hook_pre", shift_pre)],
        [("blocks.0.ln1.hook_scale", freeze_scale), ("blocks.0.ln1.hook_normalized", half), ("blocks.0.attn.hook_q", half),
         ("blocks.0.ln2.hook_scale", half), ("blocks.0.mlp.hook_pre", kill_neurons), ("blocks.0.mlp.hook_post", half)],
        [(lambda n: n.endswith(("ln1.hook_scale", "ln2.hook_normalized", "mlp.hook_pre")), half)],
        [("blocks.0.attn.hook_pattern", no_cls_attention)],
        [(f"blocks.{nl - 1}.attn.hook_attn_scores", mask_scores)],
        [("blocks.0.attn.hook_attn_scores", nan_row), ("blocks.0.attn.hook_pattern", half)],
        [("blocks.1.attn.hook_q", half), ("blocks.1.attn.hook_attn_scores", mask_scores), ("blocks.1.attn.hook_pattern", no_cls_attention),
         ("blocks.1.attn.hook_z", kill_head_1)],
        [("blocks.0.attn.hook_v", swap_heads), ("blocks.0.attn.hook_pattern", half), ("blocks.0.hook_resid_mid", half)],
        [(lambda n: n.endswith("attn.hook_pattern"), no_cls_attention)],
        [("blocks.0.attn.hook_z", kill_head_1)],
        [(f"blocks.{nl - 1}.attn.hook_z", half)],
        [("blocks.1.mlp.hook_post", kill_neurons)],
        [("blocks.0.attn.hook_q", half), ("blocks.0.attn.hook_k", kill_head_1), ("blocks.0.attn.hook_v", swap_heads)],
        [("blocks.1.attn.hook_v", swap_heads)],
        [("blocks.0.attn.hook_z", kill_head_1), ("blocks.0.hook_resid_post", half)],
        [("blocks.0.attn.hook_z", half), ("blocks.1.mlp.hook_post", kill_neurons), ("blocks.1.hook_attn_out", half)],
        [(lambda n: n.endswith("attn.hook_z"), kill_head_1)],
        [(lambda n: n.endswith(("attn.hook_q", "attn.hook_z", "hook_resid_mid", "mlp.hook_post", "hook_resid_post")), half)],
        [(f"blocks.{nl - 1}.mlp.hook_post", half), (f"blocks.{nl - 1}.hook_mlp_out", kill_head_1 if False else half)],
    ]
    # bf16: no hand-set tolerance.  The error budget of every tensor is what the PyTorch hook path of the SAME model in bf16 loses
    # against its own fp32 run under the same hooks; the HIP path's distance to that fp32 run is held to INTRA_BLOCK_RATIO x the
    # budget (tiny tensors: a few hundred elements per key, so which way single roundings fall moves the ratio; the B/32-size
    # statement against the reference's own budget is test_mutating_hooks_on_b32_vs_reference_fixture...).  A budget of exactly
    # zero (a frozen scale, a zeroed tensor) demands equality.
    ref32 = x32 = None
    if dtype == torch.bfloat16:
        m32, _, _ = build(arch_name, torch.float32)
        ref32, x32 = _pytorch_twin(m32), x.float()
    worst = [0.0, None]

    def held(a, b, b32, tag):
        if dtype == torch.float32:
            assert rel_fro(a, b) < FP32_TOL, tag
            return
        budget, err = rel_fro(b, b32), rel_fro(a, b32)
        if budget == 0.0:
            assert np.array_equal(a, b), tag
            return
        if err / budget > worst[0]:
            worst[0], worst[1] = err / budget, tag
        assert err <= INTRA_BLOCK_RATIO * budget, (tag, err, budget)

    with torch.no_grad():
        for ci, hooks in enumerate(cases):
            want = ref.run_with_hooks(x.clone(), fwd_hooks=hooks)
            got = model.run_with_hooks(x.clone(), fwd_hooks=hooks)
            assert model.last_run_native, model.native_fallback_reason
            w32 = ref32.run_with_hooks(x32.clone(), fwd_hooks=hooks).cpu().numpy() if ref32 is not None else None
            held(got.float().cpu().numpy(), want.float().cpu().numpy(), w32, (ci, "out"))
            assert all(len(hp.fwd_hooks) == 0 for hp in model.hook_dict.values())
            for kw in ({}, {"names_filter": lambda n: "resid" in n or n.endswith(("hook_z", "hook_pattern", "mlp.hook_post"))},
                       {"names_filter": lambda n: n.endswith(("hook_attn_scores", "hook_v", "hook_attn_out"))}, {"stop_at_layer": nl - 1}):
                w_out, w_cache = ref.run_with_cache(x.clone(), fwd_hooks=hooks, **kw)
                g_out, g_cache = model.run_with_cache(x.clone(), fwd_hooks=hooks, **kw)
                assert model.last_run_native, model.native_fallback_reason
                assert list(g_cache.keys()) == list(w_cache.keys())
                f_out = f_cache = None
                if ref32 is not None:
                    f_out, f_cache = ref32.run_with_cache(x32.clone(), fwd_hooks=hooks, **kw)
                    f_out = f_out.cpu().numpy()
                held(g_out.float().cpu().numpy(), w_out.float().cpu().numpy(), f_out, (ci, "out", sorted(kw)))
                for k in w_cache.keys():
                    a, b = g_cache[k].float().cpu().numpy(), w_cache[k].float().cpu().numpy()
                    # (masked / poisoned scores: -inf and NaN must sit in the same places; the norm is taken over the rest)
                    fin = np.isfinite(b)
                    assert a.shape == b.shape and np.array_equal(np.isfinite(a), fin) and np.array_equal(np.isnan(a), np.isnan(b)), (k, kw)
                    b32 = None
                    if f_cache is not None:
                        b32 = f_cache[k].float().cpu().numpy()
                        assert np.array_equal(np.isfinite(b32), fin), (k, kw)
                        b32 = np.where(fin, b32, 0.0)
                    held(np.where(fin, a, 0.0), np.where(fin, b, 0.0), b32, (ci, k, sorted(kw)))
    if dtype == torch.bfloat16:
        print(f"[intra-block hooks, bf16 {arch_name}] worst error / budget = {worst[0]:.3f} at {worst[1]}")


def test_sae_substitution_style_eval_on_b32_bf16():
    """The shape of sae/evals/evals.py:321-392 (clean / substituted / zero-ablated forward of the same batch) at the
    real size: all three run natively, substitution with the identity reproduces the clean output bit for bit."""
    model, arch, sd = build("clip-vit-b32", torch.bfloat16)
    x = torch.from_numpy(synth_images(arch, 8, 2)).cuda().bfloat16()
    name = "blocks.6.hook_resid_post"
    with torch.no_grad():
        clean, _ = model.run_with_cache(x, names_filter=[])
        assert model.last_run_native
        plain = model(x)                                               # an un-hooked no-grad forward is the same plan without taps
        assert model.last_run_native and torch.equal(plain, clean)
        same = model.run_with_hooks(x, fwd_hooks=[(name, lambda t, hook: t.clone())])
        assert model.last_run_native and torch.equal(same, clean)
        zero = model.run_with_hooks(x, fwd_hooks=[(name, lambda t, hook: torch.zeros_like(t))])
        assert model.last_run_native and not torch.equal(zero, clean)
        _, c = model.run_with_cache(x, fwd_hooks=[(name, lambda t, hook: torch.zeros_like(t))],
                                    names_filter=[name, "blocks.7.hook_resid_pre", "blocks.7.hook_resid_post"])
        assert float(c[name].abs().max()) == 0.0 and float(c["blocks.7.hook_resid_pre"].abs().max()) == 0.0
        assert float(c["blocks.7.hook_resid_post"].abs().max()) > 0.0


@pytest.mark.parametrize("tile", ["5", "4", "0"])
@pytest.mark.parametrize("M,N,K", [(700, 520, 200), (333, 264, 72), (1024, 768, 768), (97, 8, 40), (645, 264, 96), (1931, 1032, 1056),
                                   (1000, 520, 192), (2241, 776, 320)])
@pytest.mark.parametrize("loop", [-1, 0, 2])
def test_bf16_gemm_kernels_on_ragged_shapes(tile, M, N, K, loop, tuning):
    """pv_gemm_bias against an fp32 torch reference on shapes that are multiples of nothing: partial row / column
    tiles, K that ends inside a 64-byte slab (K = 200, 72, 40: the barrier-then-fetch loop) or is a whole number of
    slabs not divisible by the 4-step unrolling (K = 96, 1056: the software-pipelined loop unless gemm_loop = 0),
    N = 8 (one 16-byte chunk); K = 192, 320, 768: whole 128-byte slabs, an odd number of them too (the full-line loop)."""
    import ctypes as C
    tuning("gemm_tile", int(tile))
    tuning("gemm_loop", loop)
    L = _native.lib()
    g = torch.Generator(device="cuda").manual_seed(M * 31 + N)
    A = torch.randn(M, K, device="cuda", generator=g).bfloat16()
    Bt = torch.randn(N, K, device="cuda", generator=g).bfloat16()
    bias = torch.randn(N, device="cuda", generator=g).bfloat16()
    out = torch.full((M + 1, N), 7.0, device="cuda", dtype=torch.bfloat16)            # the extra row must stay untouched
    st = torch.cuda.current_stream().cuda_stream
    _native.check(L.pv_gemm_bias(1, A.data_ptr(), K, Bt.data_ptr(), K, bias.data_ptr(), out.data_ptr(), N, M, N, K, st), "pv_gemm_bias")
    torch.cuda.synchronize()
    ref = A.float() @ Bt.float().T + bias.float()
    err = float((out[:M].float() - ref).abs().max()) / float(ref.abs().max())
    assert err <= 2 ** -7, err                                                         # one bf16 rounding of the result
    assert float(out[M].float().min()) == 7.0 and float(out[M].float().max()) == 7.0


# ---------------------------------------------------------------------------------------------------
# parity at the configurations bench.py reports (no kernel overrides: the library picks what the bench runs)
# ---------------------------------------------------------------------------------------------------
def _held_to_budget(cache, c_ref, budget, sub, tag, scale_slack=SCALE_SLACK_BENCH, ln_taps=False):
    bad = []
    for k, ref in c_ref.items():
        got = cache[k][sub].float().cpu().numpy()
        assert got.shape == ref.shape, (tag, k)
        err = rel_fro(got, ref)
        if err > bf16_limit(k, budget[k]["rel_fro"], scale_slack, ln_taps):
            bad.append((k, err, budget[k]["rel_fro"]))
    assert not bad, (tag, bad[:8], len(bad))


def test_bf16_bs512_all_hooks_and_harvest_vs_oracle_at_reference_budget():
    """BASELINE config 2 exactly as bench.py runs it (bs = 512, bf16, all 214 hooks, the kernels the library picks at
    this size): images 0-7 and 504-511 of the batch against the fp32 oracle run on those 16 images (images do not
    interact), every key held to the error the REFERENCE's bf16 path has on the same images
    (tests/golden/vit_b32_bf16_budget_sub512.json, generated by executing the reference).  Then the harvest form of
    VisionActivationsStore.get_activations (stop_at_layer = 7, names_filter = [blocks.6.hook_resid_post])."""
    with open(os.path.join(GOLDEN, "vit_b32_bf16_budget_sub512.json")) as f:
        G = json.load(f)
    sub = G["images"]
    model, arch, sd = build("clip-vit-b32", torch.bfloat16)
    assert _native.get_tuning("any") == 0
    imgs = synth_images(arch, 512, G["seed"])
    o_ref, c_ref = vit_forward(sd, arch, imgs[sub])
    x = torch.from_numpy(imgs).cuda().bfloat16()
    with torch.no_grad():
        out, cache = model.run_with_cache(x)
        torch.cuda.synchronize()
        assert model.last_run_native and list(cache.keys()) == list(c_ref.keys()) and len(cache) == 214
        _held_to_budget(cache, c_ref, G["budget"], sub, "all hooks")
        assert rel_fro(out[sub].float().cpu().numpy(), o_ref) <= G["budget"]["__out__"]["rel_fro"] * BF16_SLACK
        del cache
        h_ref, hc_ref = vit_forward(sd, arch, imgs[sub], stop_at_layer=7, names_filter=["blocks.6.hook_resid_post"])
        hout, hcache = model.run_with_cache(x, stop_at_layer=7, names_filter=["blocks.6.hook_resid_post"])
        torch.cuda.synchronize()
        assert model.last_run_native and list(hcache.keys()) == ["blocks.6.hook_resid_post"]
        _held_to_budget(hcache, hc_ref, G["harvest"], sub, "harvest")
        assert torch.equal(hout, hcache["blocks.6.hook_resid_post"])


def test_bf16_l14_bs128_pattern_vs_oracle_at_reference_budget():
    """BASELINE config 5 as bench.py runs it (L/14@336, bs = 128, bf16, the 24 pattern taps): blocks.{0,23}.attn.hook_pattern
    of images 0 and 127 against the fp32 oracle, held to the reference's own bf16 error on the same images
    (tests/golden/vit_l14_bf16_budget_sub128.json; attention.py:135-152 is what the kernel matches)."""
    with open(os.path.join(GOLDEN, "vit_l14_bf16_budget_sub128.json")) as f:
        G = json.load(f)
    sub = G["images"]
    model, arch, sd = build("clip-vit-l14-336", torch.bfloat16)
    imgs = synth_images(arch, 128, G["seed"])
    want = [f"blocks.{l}.attn.hook_pattern" for l in (0, 23)]
    o_ref, c_ref = vit_forward(sd, arch, imgs[sub], names_filter=want)
    x = torch.from_numpy(imgs).cuda().bfloat16()
    with torch.no_grad():
        out, cache = model.run_with_cache(x, names_filter=lambda n: n.endswith("attn.hook_pattern"))
    torch.cuda.synchronize()
    assert model.last_run_native and len(cache) == 24
    _held_to_budget({k: cache[k] for k in want}, c_ref, G["budget"], sub, "l14 pattern")
    assert rel_fro(out[sub].float().cpu().numpy(), o_ref) <= G["budget"]["__out__"]["rel_fro"] * BF16_SLACK
    s = cache["blocks.23.attn.hook_pattern"][sub].float().sum(-1)
    assert float((s - 1).abs().max()) < 2e-2


def _digests(model, bs_list):
    import hashlib
    out = []
    for bs in bs_list:
        x = torch.randn(bs, 3, 224, 224, device="cuda", generator=torch.Generator(device="cuda").manual_seed(bs)).bfloat16()
        with torch.no_grad():
            o, cache = model.run_with_cache(x)
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for k in cache.keys():
            h.update(cache[k].contiguous().view(torch.uint8).cpu().numpy().tobytes())
        h.update(o.contiguous().view(torch.uint8).cpu().numpy().tobytes())
        out.append(h.hexdigest())
        del o, cache
    return out


def test_bf16_results_do_not_depend_on_the_gemm_kernel_or_the_batch_size(tuning):
    """At 77 and 300 images (partial row tiles in every GEMM) the three bf16 GEMM kernels -- 128 x 128 (v4), 256 x 256 and
    320 x 256 (v7) -- must give BIT-identical digests over all 214 cache tensors: they accumulate every output element
    in the same K order and share one activation / rounding sequence (act_any in gemm_epi.hpp).  Consequence, checked last:
    an image's cache rows are the same bits at bs = 1 (v4 picked) and inside a 300-image batch (v7 picked)."""
    model, arch, _ = build("clip-vit-b32", torch.bfloat16)
    ref = None
    # loop -1: auto (every K of this model is whole 128-byte slabs: the full-line form, persistent where it pays), 0: barrier-then-
    # fetch, 1: pipelined 64-byte slabs, 2: as auto
    for tile, loop in ((None, -1), (0, -1), (4, -1), (5, -1), (4, 0), (5, 0), (4, 1), (5, 1), (4, 2), (5, 2)):
        tuning("reset")
        if tile is not None:
            tuning("gemm_tile", tile)
        tuning("gemm_loop", loop)
        d = _digests(model, (77, 300))
        ref = ref or d
        assert d == ref, (tile, loop)
    for persist in (0, 1):                         # the persistent form (gemm_kernel_v8) wherever it applies / nowhere; default: where tiles > CUs
        tuning("reset")
        tuning("gemm_persist", persist)
        assert _digests(model, (77, 300)) == ref, ("gemm_persist", persist)
    tuning("reset")
    x = torch.randn(300, 3, 224, 224, device="cuda", generator=torch.Generator(device="cuda").manual_seed(300)).bfloat16()
    with torch.no_grad():
        _, big = model.run_with_cache(x)
        _, one = model.run_with_cache(x[123:124])
    for k in big.keys():
        assert torch.equal(big[k][123], one[k][0]), k


@pytest.mark.parametrize("epi,M,N_,K", [("bias", 25600, 2304, 768), ("act", 25600 - 37, 1000, 1024), ("resid", 8000 + 13, 1024, 256),
                                       ("resid", 25600, 768, 3072), ("act", 4 * 577, 4096, 1024), ("bias", 300, 768, 768)])
def test_persistent_gemm_is_bit_identical_to_the_one_tile_per_workgroup_form(epi, M, N_, K, tuning):
    """gemm_kernel_v8 (one workgroup per CU walking its tiles, the K slabs of consecutive tiles as one stream: DESIGN.md 3.6) against
    gemm_kernel_v7 through pv_gemm_epilogue on the forward's shapes, ragged ones and a launch smaller than the chip, for the three
    epilogue families (second output included): same MFMA order, same k order of every fp32 sum -> the same bits; and against a
    torch fp32 product of the same bf16 operands within bf16 rounding of the result (2^-8 relative to the row's largest entry)."""
    from vit_prisma_amd import _native as N
    L = N.lib()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(M + N_ + K)
    A = torch.randn(M, K, device="cuda", generator=g).bfloat16()
    B = (torch.randn(N_, K, device="cuda", generator=g) * 0.05).bfloat16()
    bias = torch.randn(N_, device="cuda", generator=g).bfloat16()
    res = torch.randn(M, N_, device="cuda", generator=g).bfloat16() if epi == "resid" else None
    outs = []
    for persist in (0, 1):
        tuning("reset")
        tuning("gemm_persist", persist)
        o0 = torch.zeros(M, N_, device="cuda", dtype=torch.bfloat16)
        o1 = torch.zeros_like(o0) if epi != "bias" else None
        N.check(L.pv_gemm_epilogue(1, {"bias": 0, "resid": 2, "act": 3}[epi], 0, A.data_ptr(), K, B.data_ptr(), K, bias.data_ptr(),
                                   res.data_ptr() if res is not None else None, N_, o0.data_ptr(), o1.data_ptr() if o1 is not None else None,
                                   N_, M, N_, K, st), "pv_gemm_epilogue")
        torch.cuda.synchronize()
        outs.append((o0, o1))
    for a, b in zip(*outs):
        if a is not None:
            assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    rows = slice(0, min(M, 512))
    pre = A[rows].float() @ B.float().T + bias.float()

    def close(got, want):
        return float(((got.float() - want).abs().amax(dim=1) / want.abs().amax(dim=1)).max()) < 2.0 ** -7

    assert close(outs[1][0][rows], pre)               # out0: the product + bias (hook_attn_out / hook_mlp_out / mlp.hook_pre; epi 0: the output)
    if epi == "resid":
        assert close(outs[1][1][rows], pre + res[rows].float())            # out1: the residual stream
    if epi == "act":
        assert close(outs[1][1][rows], torch.nn.functional.gelu(outs[1][0][rows].float()))     # out1 = act(round_T(acc + bias)), PV_ACT_GELU


def test_repeated_calls_reuse_the_host_side_plan_and_stay_exact():
    """The host side of a repeated call is cached (tap layout per (names, batch, segment), the ctypes tap array per slab, the parameter
    slots of the weight-change check): calls with different name filters, batch sizes and stop layers interleaved, entries of an
    earlier call still held (so the arena hands out another slab), and an in-place weight edit in between must give exactly what a
    fresh model gives; keys and order as always."""
    model, arch, _ = build("clip-vit-b32", torch.bfloat16)
    fresh, _, _ = build("clip-vit-b32", torch.bfloat16)
    g = torch.Generator(device="cuda").manual_seed(3)
    xa = torch.randn(5, 3, 224, 224, device="cuda", generator=g).bfloat16()
    xb = torch.randn(9, 3, 224, 224, device="cuda", generator=g).bfloat16()
    calls = [(xa, {}), (xb, {}), (xa, {"names_filter": lambda n: n.endswith("hook_resid_post")}), (xa, {}),
             (xb, {"names_filter": ["blocks.3.attn.hook_pattern", "blocks.0.hook_resid_pre"], "stop_at_layer": 5}), (xa, {}), (xb, {})]
    held = []
    with torch.no_grad():
        for rnd in range(2):
            for x, kw in calls:
                out, cache = model.run_with_cache(x, **kw)
                assert model.last_run_native
                nv = fresh._native
                if nv is not None:                                  # a fresh engine state for the comparison: no caches
                    nv._layouts.clear(); nv._tap_arrays.clear(); nv._param_slots = None
                want_out, want = fresh.run_with_cache(x, **kw)
                assert list(cache.keys()) == list(want.keys())
                assert torch.equal(out, want_out)
                for k in want.keys():
                    assert torch.equal(cache[k], want[k]), k
                held.append(cache)                                  # (keeps the slab busy: the next call gets another one)
                if len(held) > 3:
                    held.pop(0)
            # an in-place edit of a weight must reach the next call of BOTH models' engines (version counter of the parameter)
            for m in (model, fresh):
                m.blocks[2].mlp.b_out.mul_(1.5)
    assert len(model._native._layouts) >= 4 and len(model._native._tap_arrays) >= 4


def test_plain_forward_is_native_and_the_autograd_fallback_warns_once():
    model, arch, sd = build("tiny", torch.float32)
    model.use_native(None)                                             # auto mode
    x = torch.from_numpy(synth_images(arch, 2, 1)).cuda()
    with torch.no_grad():
        out = model(x)
        assert model.last_run_native
        o_ref, _ = vit_forward(sd, arch, synth_images(arch, 2, 1))
        assert rel_fro(out.cpu().numpy(), o_ref) < FP32_TOL
        mid = model(x, stop_at_layer=1)
        assert model.last_run_native and mid.shape == (2, 17, 64)
    import warnings
    with warnings.catch_warnings(record=True) as w:                    # parameters require grad, no no_grad(): PyTorch path + ONE warning
        warnings.simplefilter("always")
        out2 = model(x)
        model.run_with_cache(x)
        assert not model.last_run_native and "autograd" in model.native_fallback_reason and out2.requires_grad
    assert sum("PyTorch path" in str(m.message) for m in w) == 1


def _hook_cases():
    def scale_shift(t, hook):
        return t * 0.5 + 1.0

    def zero(t, hook):
        return torch.zeros_like(t)

    def edit_cls(t, hook):
        t[:, 0] = 0.25

    def kill_head_3(t, hook):                 # [B, T, H, dh], in place
        t[:, :, 3] = 0.0

    def no_cls_attention(t, hook):            # pattern [B, H, T, T]
        t = t.clone()
        t[..., 0] = 0.0
        return t / t.sum(-1, keepdim=True).clamp_min(1e-6)

    def mask_last_key(t, hook):               # scores [B, H, T, T], in place
        t[:, 0, :, -1] = float("-inf")

    def kill_neurons(t, hook):                # [B, T, d_mlp], in place
        t[..., ::3] = 0.0

    def freeze_scale(t, hook):                # [B, T, 1]
        return torch.full_like(t, 2.0)

    # (the same functions as tests/golden/gen_golden_vit_hooks.py ran through the REFERENCE)
    return {"A": [("blocks.6.hook_resid_post", scale_shift)],
            "B": [("blocks.3.hook_attn_out", zero), ("blocks.9.hook_resid_mid", edit_cls)],
            "C": [("blocks.5.attn.hook_z", kill_head_3)],
            "D": [("blocks.4.attn.hook_pattern", no_cls_attention)],
            "E": [("blocks.7.attn.hook_attn_scores", mask_last_key)],
            "F": [("blocks.8.mlp.hook_post", kill_neurons)],
            "G": [("blocks.2.ln1.hook_scale", freeze_scale)]}


def test_mutating_hooks_on_b32_vs_reference_fixture_fp32_and_bf16_budget():
    """SURVEY.md 8f row 1 at the real size: run_with_cache(fwd_hooks=[replacing / ablating / in-place hooks]) on the split
    native plan against what the REFERENCE produced for the same hooks (tests/golden/vit_b32_hooks_bs4.json, generated by
    executing it): fp32 fingerprints at 1e-4, bf16 held to the reference's own bf16 error under the same hooks.  Cases A / B
    hook the residual stream; C-G hook INSIDE a block (pv_vit_forward_stage: head ablation on attn.hook_z, an edited and
    renormalised attn.hook_pattern, a -inf mask on attn.hook_attn_scores, neuron ablation on mlp.hook_post, a frozen
    ln1.hook_scale -- hook_point.py:44-45, attention.py:135-152, 267-281)."""
    with open(os.path.join(GOLDEN, "vit_b32_hooks_bs4.json")) as f:
        G = json.load(f)
    m32, arch, _ = build("clip-vit-b32", torch.float32)
    m16, _, _ = build("clip-vit-b32", torch.bfloat16)
    imgs = synth_images(arch, G["batch"], G["seed"])
    cases = _hook_cases()
    assert sorted(cases) == sorted(G["cases"])
    for name, hooks in cases.items():
        want = G["cases"][name]
        keys = want.get("keys", G["keys"])
        out, cache = run(m32, imgs, torch.float32, fwd_hooks=hooks, names_filter=keys)
        assert list(cache.keys()) == keys
        for k in keys + ["__out__"]:
            got = (out if k == "__out__" else cache[k]).cpu().numpy()
            fp, gw = fingerprint(got), (want["out"] if k == "__out__" else want["cache"][k])
            assert fp["shape"] == gw["shape"], (name, k)
            assert abs(fp["l2"] - gw["l2"]) <= FP32_TOL * max(gw["l2"], 1e-6), (name, k)
            vw = np.array(gw["vals"])
            assert np.max(np.abs(np.array(fp["vals"]) - vw)) <= 1e-3 * max(np.max(np.abs(vw)), gw["l2"] / np.sqrt(got.size), 1e-6), (name, k)
        out16, cache16 = run(m16, imgs, torch.bfloat16, fwd_hooks=hooks, names_filter=keys)
        for k in keys + ["__out__"]:
            ref = (out if k == "__out__" else cache[k]).cpu().numpy()
            got = (out16 if k == "__out__" else cache16[k]).float().cpu().numpy()
            budget = want["bf16_budget"][k]
            if budget == 0.0:
                assert np.array_equal(got, ref), (name, k)               # the zero-ablated tensor / the frozen scale itself
            else:
                # (4-image fixture with a rewritten residual stream: hook_scale held to the round-2 bar of 1.25 x here)
                assert rel_fro(got, ref) <= bf16_limit(k, budget, 1.25), (name, k, rel_fro(got, ref), budget)
        if name == "E":       # the masked key gets exactly zero attention from head 0, in both modes
            for c in (cache, cache16):
                pat = c["blocks.7.attn.hook_pattern"]
                assert float(pat[:, 0, :, -1].abs().max()) == 0.0 and float(pat[:, 1, :, -1].abs().max()) > 0.0


@pytest.mark.parametrize("image_size,patch", [(224, 16), (208, 13), (400, 16), (176, 16), (256, 16), (336, 14)])
def test_bf16_long_sequence_attention_kernel(image_size, patch):
    """The T > 64 bf16 attention kernel on token counts other than L/14's 577: T = 197 (odd: head blocks of the taps only
    2-byte aligned, one full tap window + a ragged one), 257 (one key past a tile edge), 626 (> 4 windows, last one ragged),
    122 (even, < one window), 257 again at another patch size, and 577 itself.  scores / pattern / z against an fp32 recompute from the
    q, k, v the same run cached."""
    cfg = dict(n_layers=1, d_model=128, n_heads=2, d_head=64, d_mlp=256, patch_size=patch, image_size=image_size, n_channels=3,
               n_classes=16, eps=1e-5, layer_norm_pre=True, normalize_output=True, return_type="class_logits",
               activation_name="gelu", use_cls_token=True, normalization_type="LN", classification_type="cls")
    model = HookedViT(HookedViTConfig(**cfg, dtype=torch.bfloat16, device="cuda")).to(torch.bfloat16).cuda().eval().use_native(True)
    T = (image_size // patch) ** 2 + 1
    x = torch.randn(3, 3, image_size, image_size, device="cuda", generator=torch.Generator(device="cuda").manual_seed(T)).bfloat16()
    with torch.no_grad():
        _, cache = model.run_with_cache(x)
        _, only_z = model.run_with_cache(x, names_filter="blocks.0.attn.hook_z")           # no taps at all
        _, pat_z = model.run_with_cache(x, names_filter=lambda n: n.endswith(("attn.hook_pattern", "attn.hook_z")))   # no score tap
    assert model.last_run_native
    q, k, v = (cache["blocks.0.attn." + n].float() for n in ("hook_q", "hook_k", "hook_v"))
    s_ref = torch.einsum("bqhd,bkhd->bhqk", q, k) / 8.0
    s_got = cache["blocks.0.attn.hook_attn_scores"].float()
    assert s_got.shape == (3, 2, T, T)
    assert float((s_got - s_ref).abs().max()) <= 2 ** -8 * float(s_ref.abs().max()) + 1e-6
    p_got = cache["blocks.0.attn.hook_pattern"].float()
    assert float((p_got - torch.softmax(s_got, dim=-1)).abs().max()) <= 2 ** -8
    # per element, relative: 2^-8 p + 1e-30 (tests/_attention_cases.py) -- every element here is below the absolute bound
    assert pattern_elementwise_ok(p_got, torch.softmax(s_got, dim=-1))[0], pattern_elementwise_ok(p_got, torch.softmax(s_got, dim=-1))[1]
    z_ref = torch.einsum("bhqk,bkhd->bqhd", p_got, v)
    z_got = cache["blocks.0.attn.hook_z"].float()
    assert float((z_got - z_ref).abs().max()) <= 2 ** -8 * float(z_ref.abs().max()) + 1e-6
    # without the score tap: the same statements against the same fp32 recompute, and the same z whichever taps are taken
    p2 = pat_z["blocks.0.attn.hook_pattern"].float()
    assert p2.shape == (3, 2, T, T) and float((p2 - torch.softmax(s_got, dim=-1)).abs().max()) <= 2 ** -8
    assert pattern_elementwise_ok(p2, torch.softmax(s_got, dim=-1))[0]
    z2 = pat_z["blocks.0.attn.hook_z"].float()
    assert float((z2 - torch.einsum("bhqk,bkhd->bqhd", p2, v)).abs().max()) <= 2 ** -8 * float(z_ref.abs().max()) + 1e-6
    assert torch.equal(only_z["blocks.0.attn.hook_z"], pat_z["blocks.0.attn.hook_z"])
    assert torch.equal(only_z["blocks.0.attn.hook_z"], cache["blocks.0.attn.hook_z"])


def test_hooked_sae_vit_splices_run_on_the_plan_vs_reference_fixture():
    """HookedSAEViT (base_vit.py:827-1086) on the GPU: SAEs spliced in place of a block's HookPoints are served by the HIP plan (split
    there, the SAE called on the tapped tensor) -- outputs, cache keys and the tensors around the splice of the reference's own run
    (tests/golden/sae_vit_tiny.npz) with one SAE attached, two, one removed, all removed; a splice the plan cannot serve takes the
    PyTorch path and says why."""
    from vit_prisma_amd import HookedSAEViT
    from vit_prisma_amd.sae import StandardSparseAutoencoder, VisionModelSAERunnerConfig
    from vit_prisma_amd.synth import synth_sae_state
    G = np.load(os.path.join(GOLDEN, "sae_vit_tiny.npz"))
    arch = ARCHS["tiny"]
    model = HookedSAEViT(HookedViTConfig(**arch, dtype=torch.float32, device="cuda"))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth_vit_state(arch, 0).items()}, strict=True)
    model = model.cuda().eval().use_native(True)
    x = torch.from_numpy(synth_images(arch, 2, 1)).cuda()

    def make_sae(layer, subtype, act, kw, seed):
        cfg = VisionModelSAERunnerConfig(hook_point_layer=layer, layer_subtype=subtype, d_in=arch["d_model"], expansion_factor=4,
                                         activation_fn_str=act, activation_fn_kwargs=kw, normalize_activations="layer_norm",
                                         initialization_method="independent", b_dec_init_method="mean", _device="cuda", _dtype="float32",
                                         log_to_wandb=False, use_ghost_grads=False, verbose=False)
        sae = StandardSparseAutoencoder(cfg).cuda().eval()
        with torch.no_grad():
            for name, val in synth_sae_state(arch["d_model"], arch["d_model"] * 4, seed=seed).items():
                getattr(sae, name).copy_(torch.from_numpy(val))
        return sae

    def check(tag):
        with torch.no_grad():
            out, cache = model.run_with_cache(x)
        assert model.last_run_native, model.native_fallback_reason
        assert list(cache.keys()) == [str(k) for k in G[f"{tag}_keys"]], tag
        assert rel_fro(out.cpu().numpy(), G[f"{tag}_out"]) < FP32_TOL, tag
        for key in G.files:
            if key.startswith(tag + "::"):
                name = key.split("::", 1)[1]
                assert cache[name].shape == G[key].shape and rel_fro(cache[name].cpu().numpy(), G[key]) < FP32_TOL, key
        return out

    out0 = check("plain")
    a = make_sae(0, "hook_resid_post", "relu", {}, 3)
    b = make_sae(1, "hook_mlp_out", "topk", {"k": 8}, 4)
    model.add_sae(a)
    check("one")
    with torch.no_grad():
        plain_call = model(x)                                        # no caching: the SAE runs on its own HIP engine inside the split
        assert model.last_run_native and rel_fro(plain_call.cpu().numpy(), G["one_forward"]) < FP32_TOL
    model.add_sae(b)
    check("two")
    model.reset_saes(a.cfg.hook_point)
    check("only_b")
    model.reset_saes()
    assert torch.equal(check("reset"), out0)
    # a splice on block 0's entry: that block on its own module, the rest on the plan -- against the REFERENCE's own run of that splice
    # (tests/golden/sae_vit_tiny_edges.npz), and the same numbers as the PyTorch path
    E = np.load(os.path.join(GOLDEN, "sae_vit_tiny_edges.npz"))
    e = make_sae(0, "hook_resid_pre", "relu", {}, 5)
    model.add_sae(e)

    def check_edge(tag):
        with torch.no_grad():
            out_n, c_n = model.run_with_cache(x)
            assert model.last_run_native
            model.use_native(False)
            out_t, c_t = model.run_with_cache(x)
            model.use_native(True)
        assert list(c_n.keys()) == list(c_t.keys()) == [str(k) for k in E[f"{tag}::__keys__"]]
        assert rel_fro(out_n.cpu().numpy(), E[f"{tag}::__out__"]) < FP32_TOL and rel_fro(out_t.cpu().numpy(), E[f"{tag}::__out__"]) < FP32_TOL
        for k in c_t.keys():
            assert rel_fro(c_n[k].cpu().numpy(), E[f"{tag}::{k}"]) < FP32_TOL, k

    check_edge("entry0")
    model.reset_saes()
    # cfg.hook_point = ... does NOT move an SAE: the reference's setter stores a value its getter never reads (sae/config.py:428-436);
    # the fixture's "embed" case is the reference after that assignment -- the same splice as before
    e.cfg.hook_point = "hook_embed"
    assert e.cfg.hook_point == "blocks.0.hook_resid_pre"
    model.add_sae(e)
    check_edge("embed")
    model.reset_saes()
    # on the embedding stage (reachable with a config CLASS whose hook point is something else: not through the reference's config):
    # that stage on the model's own modules, the blocks on the plan
    e.cfg.__class__ = type("EmbedStageCfg", (type(e.cfg),), {"hook_point": "hook_embed"})
    model.add_sae(e)
    with torch.no_grad():
        out_n, c_n = model.run_with_cache(x)
        assert model.last_run_native
        model.use_native(False)
        out_t, c_t = model.run_with_cache(x)
        model.use_native(True)
    assert list(c_n.keys()) == list(c_t.keys()) and "hook_embed.hook_sae_out" in c_n and "hook_embed" not in c_n
    assert rel_fro(out_n.cpu().numpy(), out_t.cpu().numpy()) < FP32_TOL
    model.reset_saes()
    # in another dtype than the model's: the PyTorch path, and it says why
    model.use_native(None)
    model.add_sae(make_sae(1, "hook_resid_post", "relu", {}, 6).double())
    model.acts_to_saes["blocks.1.hook_resid_post"].dtype = torch.float64
    assert model._boundary_hooks() is None
    model.reset_saes()


def test_hooked_sae_vit_at_b32_size_vs_reference_fixture():
    """HookedSAEViT at CLIP ViT-B/32 size (bs = 4, fp32): a top-k SAE (768 -> 3072, k = 32) in place of blocks.6.hook_resid_post, then a ReLU
    SAE in place of blocks.3.hook_mlp_out as well -- served by the HIP plan (split at the splice, the SAE on its own HIP engine or its
    hookable forward); every one of the 217 / 220 cache entries and the output against the reference's own run of its class
    (tests/golden/sae_vit_b32_bs4.json, fingerprints; gen_golden_sae_vit.py).  Round 4 had this on the tiny model only."""
    from vit_prisma_amd import HookedSAEViT
    from vit_prisma_amd.sae import StandardSparseAutoencoder, VisionModelSAERunnerConfig
    from vit_prisma_amd.synth import synth_sae_state
    with open(os.path.join(GOLDEN, "sae_vit_b32_bs4.json")) as f:
        G = json.load(f)
    arch = ARCHS["clip-vit-b32"]
    model = HookedSAEViT(HookedViTConfig(**arch, dtype=torch.float32, device="cuda"))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth_vit_state(arch, 0).items()}, strict=True)
    model = model.cuda().eval().use_native(True)
    x = torch.from_numpy(synth_images(arch, G["batch"], G["seed"])).cuda()

    def check(tag):
        with torch.no_grad():
            out, cache = model.run_with_cache(x)
        torch.cuda.synchronize()
        assert model.last_run_native, model.native_fallback_reason
        assert list(cache.keys()) == G[tag]["keys"], tag
        for k in G[tag]["keys"]:
            want = G[tag]["cache"][k]
            got = cache[k].float().cpu().numpy()
            assert list(got.shape) == want["shape"], (tag, k)
            fp = fingerprint(got)
            assert abs(fp["l2"] - want["l2"]) <= FP32_TOL * max(want["l2"], 1e-30), (tag, k, fp["l2"], want["l2"])
            vw = np.array(want["vals"])
            assert np.max(np.abs(np.array(fp["vals"]) - vw)) <= 1e-3 * max(np.max(np.abs(vw)), want["l2"] / np.sqrt(max(got.size, 1))), (tag, k)
        fo = fingerprint(out.cpu().numpy())
        assert abs(fo["l2"] - G[tag]["out"]["l2"]) <= FP32_TOL * G[tag]["out"]["l2"], tag

    for i, (tag, spec) in enumerate(zip(("one", "two"), G["saes"])):
        cfg = VisionModelSAERunnerConfig(hook_point_layer=spec["layer"], layer_subtype=spec["subtype"], d_in=arch["d_model"], expansion_factor=4,
                                         activation_fn_str=spec["act"], activation_fn_kwargs=spec["kw"], normalize_activations="layer_norm",
                                         initialization_method="independent", b_dec_init_method="mean", _device="cuda", _dtype="float32",
                                         log_to_wandb=False, use_ghost_grads=False, verbose=False)
        sae = StandardSparseAutoencoder(cfg).cuda().eval()
        with torch.no_grad():
            for name, val in synth_sae_state(arch["d_model"], arch["d_model"] * 4, seed=spec["seed"]).items():
                getattr(sae, name).copy_(torch.from_numpy(val))
        model.add_sae(sae)
        check(tag)
    model.reset_saes()
    assert model._tree_matches()


@pytest.mark.parametrize("tag,flags", [("all", dict(use_attn_result=True, use_split_qkv_input=True, use_attn_in=True, use_hook_mlp_in=True)),
                                       ("result_mlp", dict(use_attn_result=True, use_hook_mlp_in=True))])
def test_flag_gated_hook_points_on_the_plan_vs_reference_fixture(tag, flags):
    """use_attn_result / use_split_qkv_input / use_attn_in / use_hook_mlp_in (transformer_block.py:88-129, attention.py:155-183): a caching
    run stays on the HIP plan, the flag-gated entries are derived from its taps -- keys, order, shapes, dtypes and values of the
    reference's own run (tests/golden/vit_tiny_flags.npz); a hook ON such a point sends that block to its own PyTorch module and leaves
    the others on the plan."""
    G = np.load(os.path.join(GOLDEN, "vit_tiny_flags.npz"))
    arch = ARCHS["tiny"]
    model = HookedViT(HookedViTConfig(**arch, **flags, dtype=torch.float32, device="cuda"))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth_vit_state(arch, 0).items()}, strict=True)
    model = model.cuda().eval()
    x = torch.from_numpy(synth_images(arch, 2, 1)).cuda()
    keys = [str(k) for k in G[f"{tag}::__keys__"]]
    with torch.no_grad():
        out, cache = model.run_with_cache(x)
        assert model.last_run_native, model.native_fallback_reason
        assert list(cache.keys()) == keys
        assert rel_fro(out.cpu().numpy(), G[f"{tag}::__out__"]) < FP32_TOL
        for k in keys:
            g = G[f"{tag}::{k}"]
            assert cache[k].shape == g.shape and cache[k].dtype == torch.float32, k
            assert rel_fro(cache[k].cpu().numpy(), g) < FP32_TOL, k
        # the helpers that read the per-head result
        per_head = cache.stack_head_results(layer=-1)
        assert per_head.shape[0] == arch["n_layers"] * arch["n_heads"]
        name = "blocks.0.attn.hook_result"
        hooks = [(name, lambda t, hook: t * 0.5), ("blocks.1.hook_mlp_in", lambda t, hook: t + 1.0), ("blocks.1.attn.hook_z", lambda t, hook: t * 2.0)]
        out_h, cache_h = model.run_with_cache(x, fwd_hooks=hooks)
        assert model.last_run_native, model.native_fallback_reason
        assert torch.allclose(cache_h[name], cache[name] * 0.5, rtol=1e-4, atol=1e-6)
        model.use_native(False)
        out_t, cache_t = model.run_with_cache(x, fwd_hooks=hooks)
        model.use_native(None)
        assert list(cache_h.keys()) == list(cache_t.keys()) and rel_fro(out_h.cpu().numpy(), out_t.cpu().numpy()) < FP32_TOL
        for k in cache_t.keys():
            assert cache_h[k].shape == cache_t[k].shape and rel_fro(cache_h[k].cpu().numpy(), cache_t[k].cpu().numpy()) < FP32_TOL, k


@pytest.mark.parametrize("tag", ["all", "attn_in", "result_mlp", "split"])
def test_hooks_on_flag_gated_points_vs_reference_fixture(tag):
    """Forward hooks that EDIT attn.hook_result / hook_mlp_in / hook_attn_in / hook_q_input / hook_v_input (+ an ordinary point beside
    them) against the REFERENCE's own hooked runs (tests/golden/vit_tiny_flag_hooks.npz) -- output, key order and every cache tensor --
    with EVERY block on the HIP plan (round 6, VERDICT r5 item 7: attn.hook_result / hook_mlp_in are served at the block's positions 6 / 7
    -- one einsum + the head sum, ln2 of the edited input -- and hooks on the per-head inputs run only the block's head on the module's
    code before the plan is entered at PV_STAGE_QKV; round 5 sent such a block to its PyTorch module)."""
    from test_flag_hooks_vs_reference_cpu import check_case
    check_case(tag, "cuda", FP32_TOL, expect_native=True, blocks_on_plan=True)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_flag_gated_hook_points_at_b32_size_vs_reference_fixture(dtype):
    """The four flags at CLIP ViT-B/32 size (286 cache entries per forward, bs = 2): fp32 against the reference's own run,
    fingerprinted (tests/golden/vit_b32_flags_bs2.json: key order, shapes, l2, sampled values); bf16: keys / shapes / dtypes, every entry
    held to the reference's own bf16 error with the flags on (vit_b32_flags_bf16_budget_bs2.json), and the derived entries consistent with
    what they are derived from."""
    with open(os.path.join(GOLDEN, "vit_b32_flags_bs2.json")) as f:
        G = json.load(f)
    arch = ARCHS["clip-vit-b32"]
    flags = dict(use_attn_result=True, use_split_qkv_input=True, use_attn_in=True, use_hook_mlp_in=True)
    model = HookedViT(HookedViTConfig(**arch, **flags, dtype=dtype, device="cuda"))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth_vit_state(arch, 0).items()}, strict=True)
    model = model.to(dtype).cuda().eval().use_native(True)
    x = torch.from_numpy(synth_images(arch, 2, 1)).cuda().to(dtype)
    with torch.no_grad():
        out, cache = model.run_with_cache(x)
    assert model.last_run_native and list(cache.keys()) == G["keys"] and len(cache) == 286
    H = arch["n_heads"]
    for k in G["keys"]:
        got = cache[k]
        assert list(got.shape) == G["cache"][k]["shape"], k
        if dtype == torch.float32:
            fp = fingerprint(got.cpu().numpy())
            assert abs(fp["l2"] - G["cache"][k]["l2"]) <= FP32_TOL * G["cache"][k]["l2"], k
            vw = np.array(G["cache"][k]["vals"])
            assert np.max(np.abs(np.array(fp["vals"]) - vw)) <= 1e-3 * max(np.max(np.abs(vw)), G["cache"][k]["l2"] / np.sqrt(got.numel())), k
    if dtype == torch.float32:
        fo = fingerprint(out.cpu().numpy())
        assert abs(fo["l2"] - G["out"]["l2"]) <= FP32_TOL * G["out"]["l2"]
    else:
        # bf16: EVERY one of the 286 entries against fp32 truth -- the oracle's 214 plain entries and the flag-gated ones derived from them in
        # fp32 as the reference's forward defines them (transformer_block.py:88-129, attention.py:155-183) -- held to the error the
        # REFERENCE's own bf16 run with the four flags has on the same images (tests/golden/vit_b32_flags_bf16_budget_bs2.json, generated by
        # executing the reference: gen_golden_vit_flags.py).  Round 4 only checked this mode for self-consistency.
        with open(os.path.join(GOLDEN, "vit_b32_flags_bf16_budget_bs2.json")) as f:
            B = json.load(f)["budget"]
        sd = synth_vit_state(arch, 0)
        o_ref, c_ref = vit_forward(sd, arch, synth_images(arch, 2, 1))
        Hn = arch["n_heads"]
        headed = lambda a: np.broadcast_to(a[:, :, None, :], a.shape[:2] + (Hn,) + a.shape[2:])      # noqa: E731
        bad = []
        for k in G["keys"]:
            if k.startswith("blocks."):
                _, l, rest = k.split(".", 2)
                pb = f"blocks.{l}."
                if rest in ("hook_attn_in", "hook_q_input", "hook_k_input", "hook_v_input"):
                    truth = headed(c_ref[pb + "hook_resid_pre"])
                elif rest in ("ln1.hook_scale", "ln1.hook_normalized"):
                    truth = headed(c_ref[k])
                elif rest == "hook_mlp_in":
                    truth = c_ref[pb + "hook_resid_mid"]
                elif rest == "attn.hook_result":
                    truth = np.einsum("bphd,hdm->bphm", c_ref[pb + "attn.hook_z"].astype(np.float64),
                                      sd[pb + "attn.W_O"].astype(np.float64)).astype(np.float32)
                else:
                    truth = c_ref[k]
            else:
                truth = c_ref[k]
            got = cache[k].float().cpu().numpy()
            assert got.shape == tuple(truth.shape), k
            err = rel_fro(got, truth)
            if err > bf16_limit(k, B[k]["rel_fro"]):
                bad.append((k, err, B[k]["rel_fro"]))
        assert not bad, (bad[:8], len(bad))
        assert rel_fro(out.float().cpu().numpy(), o_ref) <= B["__out__"]["rel_fro"] * BF16_SLACK
    for l in (0, 11):
        p = f"blocks.{l}."
        assert torch.equal(cache[p + "hook_attn_in"], cache[p + "hook_resid_pre"].unsqueeze(2).expand(-1, -1, H, -1))
        assert torch.equal(cache[p + "hook_mlp_in"], cache[p + "hook_resid_mid"])
        assert cache[p + "ln1.hook_scale"].dtype == torch.float32 and cache[p + "attn.hook_result"].dtype == dtype
        # the per-head results sum to the O-projection's output (attention.py:170-183), to the rounding of the storage dtype
        summed = cache[p + "attn.hook_result"].float().sum(2) + model.blocks[l].attn.b_O.detach().float()
        tol = 2e-5 if dtype == torch.float32 else 3e-2
        assert rel_fro(summed.cpu().numpy(), cache[p + "hook_attn_out"].float().cpu().numpy()) < tol, l
