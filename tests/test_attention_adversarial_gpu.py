"""Every attention kernel behind dispatch_attn on adversarial q, k, v (tests/_attention_cases.py): one-hot next to near-uniform rows with
the maxima on tile edges and in the ragged last tile, scores at +-1000, and rows with NaN / +-inf scores among good rows.  The tensors
are handed to the plan by hooks on attn.hook_q / hook_k / hook_v that return them: the block re-enters at PV_STAGE_QKV and
pv_launch_attention runs with its normal dispatch.  Bounds: the module docstring of _attention_cases.  Run with ``-m gpu`` on an MI355X.

The dispatch table (csrc/attention.hip, dispatch_attn; the body of attn_stream_kernel: csrc/attn_stream.hpp), and the (dtype, d_head, T)
that reach each entry here:

    bf16, T <= 64, T even                       attn_wave_kernel<dh>           bf16 dh 32 / 64, T = 50, 64 (64: no cls token)
    bf16, T > 64, d_head 64                     attn_lean_kernel               bf16 dh 64, T = 65, 257, 677, 1025
    otherwise T <= 64                           attn_kernel<.., 64, dh, 1>     fp32 dh 32 / 64, T = 50; bf16 dh 32 / 64, T = 17 (odd)
    otherwise T <= 640                          attn_kernel<.., 32, dh, 10>    fp32 dh 32 / 64 and bf16 dh 32, T = 65, 257, 626
    otherwise T <= 2048                         attn_stream_kernel<.., dh>     fp32 dh 32 / 64 and bf16 dh 32, T = 677, 1025;
                                                                               bf16 dh 64 under the attn_wg override (which keeps
                                                                               that shape away from attn_lean_kernel), T = 677, 1025

No tuning key or profiling tag names the attention kernel that ran (the profiler has one kind for all of them), so this table is the
contract: a change to dispatch_attn has to be followed here.  T = 2026 is left to test_dino_gpu (the cap; a float64 reference there
costs more than it tells).
"""
import functools

import pytest
import torch

from vit_prisma_amd import HookedViT, HookedViTConfig

import _attention_cases as AC

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
IMAGE = {17: (16, True), 50: (28, True), 64: (32, False), 65: (32, True), 257: (64, True), 626: (100, True), 677: (104, True),
         1025: (128, True)}                                        # T -> (image size at patch 4, cls token)

PATHS = (
    [("wave", BF16, dh, T, 0) for dh in (32, 64) for T in (50, 64)]
    + [("wg64", F32, dh, 50, 0) for dh in (32, 64)]
    + [("wg64", BF16, dh, 17, 0) for dh in (32, 64)]
    + [("wg32", dt, dh, T, 0) for dt, dh in ((F32, 32), (F32, 64), (BF16, 32)) for T in (65, 257, 626)]
    + [("lean", BF16, 64, T, 0) for T in (65, 257, 677, 1025)]
    + [("stream", dt, dh, T, wg) for dt, dh, wg in ((F32, 32, 0), (F32, 64, 0), (BF16, 32, 0), (BF16, 64, 1)) for T in (677, 1025)]
)


def _id(path):
    kernel, dtype, dh, T, wg = path
    return f"{kernel}-{'bf16' if dtype == BF16 else 'fp32'}-dh{dh}-T{T}" + ("-attn_wg" if wg else "")


@functools.lru_cache(maxsize=None)
def _model(dtype, dh, T):
    image_size, cls = IMAGE[T]
    cfg = dict(n_layers=1, d_model=2 * dh, n_heads=2, d_head=dh, d_mlp=128, patch_size=4, image_size=image_size, n_channels=3,
               n_classes=16, eps=1e-5, layer_norm_pre=True, normalize_output=True, return_type="class_logits", activation_name="gelu",
               use_cls_token=cls, normalization_type="LN", classification_type="cls")
    torch.manual_seed(T + dh)
    model = HookedViT(HookedViTConfig(**cfg, dtype=dtype, device="cuda")).to(dtype).cuda().eval().use_native(True)
    assert model.n_tokens == T
    x = torch.randn(AC.B, 3, image_size, image_size, device="cuda", generator=torch.Generator(device="cuda").manual_seed(T)).to(dtype)
    return model, x


@functools.lru_cache(maxsize=None)
def _case(name, T, dh):
    return tuple(t.cuda() for t in AC.make_case(name, T, dh))


@pytest.mark.parametrize("name", AC.CASES)
@pytest.mark.parametrize("path", PATHS, ids=_id)
def test_attention_kernels_on_adversarial_inputs(path, name, tuning):
    kernel, dtype, dh, T, wg = path
    model, x = _model(dtype, dh, T)
    q, k, v = _case(name, T, dh)
    pre = "blocks.0.attn."
    hooks = [(pre + n, (lambda t, hook=None, r=r.to(dtype): r)) for n, r in (("hook_q", q), ("hook_k", k), ("hook_v", v))]
    if wg:
        tuning("attn_wg", 1)
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
