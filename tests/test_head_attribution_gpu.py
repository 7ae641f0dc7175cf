"""pv_head_attribution (csrc/attribution.hip) on the planted inputs of tests/_attribution_cases.py, and the Python surface
(vit_prisma_amd/logit_attribution.py) on the tiny bf16 ViT and text tower.  Run with ``-m gpu`` on an MI355X.

Kernel level, per shape of _attribution_cases.SHAPES, with shared and with per-image answers, and with pos in {-1, 0, T - 1}:
  * every finite element within (2 d + d_head + 8) 2^-24 sum_e |z_e| sum_k |W_ek| (|a_k| + mean|a|) / scale of the float64 truth
  * the heads that hold a NaN or an infinity NaN in every column, and no other element NaN; the zero head exactly 0
  * per-image answers: image 1 the exact negative of image 0
  * nothing written outside [B, T_out, L H, O], everything inside written
End to end: head_logit_attribution on a run_with_cache of the tiny bf16 ViT (and once of the text tower) reports the HIP path and
agrees, under the same per-element bound, with the fallback's spelling evaluated in float64 on the same cached tensors and weights.
Refusals: 17 answers, a d_head that is neither 32 / 64 nor a wide head, a short workspace -- each its error code, nothing launched.
(The wide heads are every multiple of 8 in (64, 128]; 72 is one of them and is served -- the last shape -- while 48 and 76 are
refused.)
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from vit_prisma_amd import _native, head_logit_attribution, logit_attribution

import _attribution_cases as AC

pytestmark = pytest.mark.gpu

GUARD = 1024                 # elements of 7.0 on both sides of the output


def attribute(z, W_O, scale, answers, pos=-1, expect=0, n_answers=None, d_head=None, ws_bytes=None):
    """pv_head_attribution on taps z [L][B, T, H, dh] and W_O [L][H, dh, d] (bf16), scale [B, T] and answers [O, d] | [B, O, d]
    (fp32), all CUDA tensors, into a buffer prefilled with 7 that carries GUARD elements on both sides: (buffer, view)"""
    lib = _native.lib()
    L, (B, T, H, dh), d = len(z), z[0].shape, W_O[0].shape[-1]
    per_image = answers.dim() == 3
    O = answers.shape[-2] if n_answers is None else n_answers
    dh = dh if d_head is None else d_head
    dev = answers.device
    t_out = T if pos < 0 else 1
    n = B * t_out * L * H * O
    whole = torch.full((n + 2 * GUARD,), 7.0, dtype=torch.float32, device=dev)
    view = whole[GUARD:GUARD + n]
    need = lib.pv_head_attribution_workspace_bytes(L, H, dh, B * O if per_image else O)
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
    z_ptrs = (C.c_void_p * L)(*[t.data_ptr() for t in z])
    w_ptrs = (C.c_void_p * L)(*[t.data_ptr() for t in W_O])
    rc = lib.pv_head_attribution(_native.PV_DTYPE_BF16, z_ptrs, w_ptrs, L, B, T, pos, H, dh, d, scale.data_ptr(), answers.data_ptr(),
                                 O, 1 if per_image else 0, view.data_ptr(), ws.data_ptr(), need if ws_bytes is None else ws_bytes,
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == expect, _native.last_error()
    torch.cuda.synchronize()
    return whole, view


@functools.lru_cache(maxsize=None)
def device_inputs(shape, per_image):
    case = AC.make_case(shape, per_image)
    L = case.z.shape[0]
    z = [torch.from_numpy(case.z[l]).cuda().to(torch.bfloat16).contiguous() for l in range(L)]
    W_O = [torch.from_numpy(case.W_O[l]).cuda().to(torch.bfloat16).contiguous() for l in range(L)]
    return case, z, W_O, torch.from_numpy(case.scale).cuda(), torch.from_numpy(case.answers).cuda()


CASES = [(shape, per_image, pos) for shape in AC.SHAPES for per_image in (False, True) for pos in (-1, 0, shape[1] - 1)]


def case_id(c) -> str:
    return f"{AC.shape_id(c[0])}-{'per-image' if c[1] else 'shared'}-pos{c[2]}"


@pytest.mark.parametrize("shape,per_image,pos", CASES, ids=[case_id(c) for c in CASES])
def test_planted_cases_within_the_derived_bound(shape, per_image, pos):
    case, z, W_O, scale, answers = device_inputs(shape, per_image)
    B, T, L, H, dh, d, O = shape
    whole, view = attribute(z, W_O, scale, answers, pos=pos)
    assert bool((whole[:GUARD] == 7.0).all()) and bool((whole[-GUARD:] == 7.0).all()), "written outside the output"
    assert not bool((view == 7.0).any()), "an element inside the output was not written"
    got = view.view(B, T if pos < 0 else 1, L * H, O).cpu().numpy()
    truth, bound = AC.select_pos(case.truth, pos), AC.select_pos(case.bound, pos)
    nan, zero = AC.select_pos(case.nan, pos), AC.select_pos(case.zero, pos)
    assert np.isnan(got[nan]).all(), "a head whose z holds a NaN or an infinity must be NaN in every column"
    assert np.isfinite(got[~nan]).all(), "a non-finite head leaked into another head"
    assert (got[zero] == 0).all(), "the head whose z is zero must be exactly 0"
    live = ~nan & ~zero
    ratio = np.abs(got[live].astype(np.float64) - truth[live]) / bound[live]
    print(f"{case_id((shape, per_image, pos))}: worst |got - truth| / bound = {ratio.max():.4f}")
    assert ratio.max() <= 1.0
    if pos < 0:
        assert nan.any() and zero.any()
    if per_image:
        ok = ~nan[0]
        assert np.array_equal(got[1][ok], -got[0][ok]), "image 1 (negated answers, the same z) is not the exact negative of image 0"


def test_refusals_launch_nothing():
    case, z, W_O, scale, answers = device_inputs(AC.SHAPES[0], False)

    def untouched(whole):
        return bool((whole == 7.0).all())

    whole, _ = attribute(z, W_O, scale, answers, n_answers=17, expect=1)
    assert "16" in _native.last_error() and untouched(whole)
    for dh in (48, 76):
        whole, _ = attribute(z, W_O, scale, answers, d_head=dh, expect=1)
        assert "d_head" in _native.last_error() and untouched(whole)
    whole, _ = attribute(z, W_O, scale, answers, ws_bytes=64, expect=3)
    assert "workspace" in _native.last_error() and untouched(whole)
    whole, _ = attribute(z, W_O, scale, answers, pos=AC.SHAPES[0][1], expect=1)
    assert "pos" in _native.last_error() and untouched(whole)


# ---------------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------------
def float64_spelling(cache, answers, layer, pos):
    """(truth, bound) [B, T_out, layer * H, O] float64: the fallback's composition on float64 copies of the cached hook_z, the
    model's W_O and the cached scale, and the bound of _attribution_cases on the same operands"""
    model = cache.model
    n_layers = model.cfg.n_layers
    z = np.stack([cache[f"blocks.{l}.attn.hook_z"].float().cpu().numpy() for l in range(layer)])
    W_O = np.stack([model.blocks[l].attn.W_O.detach().float().cpu().numpy() for l in range(layer)])
    key = "ln_final.hook_scale" if layer == n_layers else f"blocks.{layer}.ln1.hook_scale"
    scale = cache[key][..., 0].cpu().numpy()
    truth, bound = AC.truth_and_bound(z, W_O, answers.float().cpu().numpy(), scale)
    return AC.select_pos(truth, -1 if pos is None else pos), AC.select_pos(bound, -1 if pos is None else pos)


def check_end_to_end(cache, d_model, n_images):
    H = cache.model.cfg.n_heads
    n_layers = cache.model.cfg.n_layers
    gen = torch.Generator().manual_seed(5)
    shared = (0.05 * torch.randn(20, d_model, generator=gen) + 0.02).cuda()              # 20 answers: two chunks
    per_image = (0.05 * torch.randn(n_images, 3, d_model, generator=gen) + 0.02).cuda()
    logit_attribution.use_native(True)
    try:
        for answers, layer, pos in ((shared, None, None), (per_image, None, 0), (shared, 1, 0), (per_image, n_layers, None)):
            with torch.no_grad():
                got, labels = head_logit_attribution(cache, answers, layer=layer, pos=pos)
            assert logit_attribution.last_run_native, logit_attribution.native_fallback_reason
            lay = n_layers if layer is None else layer
            assert labels == [f"L{l}H{h}" for l in range(lay) for h in range(H)]
            truth, bound = float64_spelling(cache, answers, lay, pos)
            assert got.dtype == torch.float32 and tuple(got.shape) == truth.shape
            ratio = np.abs(got.cpu().numpy().astype(np.float64) - truth) / bound
            print(f"layer={layer} pos={pos} answers={tuple(answers.shape)}: worst |HIP - float64| / bound = {ratio.max():.4f}")
            assert np.isfinite(ratio).all() and ratio.max() <= 1.0
            # the PyTorch path of the same call: the same numbers up to the bf16 rounding of its intermediates
            logit_attribution.use_native(False)
            with torch.no_grad():
                ref = head_logit_attribution(cache, answers, layer=layer, pos=pos, return_labels=False)
            assert not logit_attribution.last_run_native and ref.shape == got.shape and ref.dtype == got.dtype
            logit_attribution.use_native(True)
    finally:
        logit_attribution.use_native(None)


def test_tiny_vit_end_to_end():
    from test_native_vit_gpu import build, run
    from vit_prisma_amd.synth import synth_images
    model, arch, _ = build("tiny", torch.bfloat16)
    _, cache = run(model, synth_images(arch, 2, 1), torch.bfloat16)
    check_end_to_end(cache, arch["d_model"], 2)


def test_tiny_text_tower_end_to_end():
    from test_text_tower_cpu import BATCH, tiny_text_model
    from vit_prisma_amd.synth import ARCHS, synth_tokens
    model = tiny_text_model(torch.bfloat16, "cuda").use_native(True)
    with torch.no_grad():
        _, cache = model.run_with_cache(torch.from_numpy(synth_tokens(ARCHS["tiny-text"], BATCH, seed=1)).cuda())
    assert model.last_run_native, model.native_fallback_reason
    check_end_to_end(cache, ARCHS["tiny-text"]["d_model"], BATCH)
