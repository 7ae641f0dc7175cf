"""pv_neuron_attribution and pv_neuron_attribution_topk (csrc/attribution_neuron.hip) on the planted inputs of
tests/_neuron_attribution_cases.py, and the Python surface (vit_prisma_amd/logit_attribution.py) on the tiny bf16 ViT and text
tower.  Run with ``-m gpu`` on an MI355X.

Dense, per shape of _neuron_attribution_cases.SHAPES, with shared and with per-image answers, and with pos in {-1, 0, T - 1}:
  * every finite element within (2 d + 8) 2^-24 |post| sum_k |W_nk| (|a_k| + mean|a|) / scale of the float64 truth
  * the neurons whose post is a NaN or an infinity NaN in every column, and no other element NaN; zeros exactly 0
  * per-image answers: image 1 the exact negative of image 0
  * nothing written outside [B, T_out, L M, O], everything inside written
Top-k, for k in {1, 2, 3, 16, 256} (capped at L M) x by in {0, 1}, and k = L M on the smallest shape: idx equals the oracle
(_neuron_attribution_cases.topk_order) applied to the dense kernel's OWN output on the same inputs, exactly -- the tie token at
k = 2, 3, the mass tie of +-0 of the sparse token (the radix-select path where L M > 1024) and the NaN-first order included --
and val equals that output gathered at idx, compared as uint32; the guards of both outputs untouched.
End to end: neuron_logit_attribution / top_neuron_logit_attribution on a run_with_cache of the tiny bf16 ViT (and once of the text
tower) report the HIP path; the dense result agrees, under the same per-element bound, with the float64 spelling on the cached
tensors; layer * d_mlp + neuron of the top-k equals the oracle on the HIP dense result.
Refusals launch nothing.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from vit_prisma_amd import _native, logit_attribution, neuron_logit_attribution, top_neuron_logit_attribution

import _neuron_attribution_cases as NC

pytestmark = pytest.mark.gpu

GUARD = 1024                 # elements of 7 on both sides of every output


def _head(lib, post, W_out, scale, answers, pos, n_answers, d_mlp):
    L, (B, T, M), d = len(post), post[0].shape, W_out[0].shape[-1]
    per_image = answers.dim() == 3
    O = answers.shape[-2] if n_answers is None else n_answers
    M = M if d_mlp is None else d_mlp
    need = lib.pv_neuron_attribution_workspace_bytes(L, M, B * O if per_image else O)
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device=answers.device)
    p_ptrs = (C.c_void_p * L)(*[t.data_ptr() for t in post])
    w_ptrs = (C.c_void_p * L)(*[t.data_ptr() for t in W_out])
    args = (_native.PV_DTYPE_BF16, p_ptrs, w_ptrs, L, B, T, pos, M, d, scale.data_ptr(), answers.data_ptr(), O, 1 if per_image else 0)
    return args, ws, need, (B, T if pos < 0 else 1, L * post[0].shape[-1], answers.shape[-2])


def dense(post, W_out, scale, answers, pos=-1, expect=0, n_answers=None, d_mlp=None, ws_bytes=None):
    """pv_neuron_attribution on taps post [L][B, T, M] and W_out [L][M, d] (bf16), scale [B, T] and answers [O, d] | [B, O, d] (fp32),
    all CUDA tensors, into a buffer prefilled with 7 that carries GUARD elements on both sides: (buffer, view)"""
    lib = _native.lib()
    args, ws, need, (B, t_out, C_, O) = _head(lib, post, W_out, scale, answers, pos, n_answers, d_mlp)
    n = B * t_out * C_ * O
    whole = torch.full((n + 2 * GUARD,), 7.0, dtype=torch.float32, device=answers.device)
    view = whole[GUARD:GUARD + n]
    rc = lib.pv_neuron_attribution(*args, view.data_ptr(), ws.data_ptr(), need if ws_bytes is None else ws_bytes,
                                   torch.cuda.current_stream().cuda_stream)
    assert rc == expect, _native.last_error()
    torch.cuda.synchronize()
    return whole, view.view(B, t_out, C_, O)


def topk(post, W_out, scale, answers, k, by, pos=-1, expect=0):
    """pv_neuron_attribution_topk into two guarded buffers prefilled with 7: (val buffer, idx buffer, val view, idx view)"""
    lib = _native.lib()
    args, ws, need, (B, t_out, _, O) = _head(lib, post, W_out, scale, answers, pos, None, None)
    n = B * t_out * O * max(k, 1)
    val = torch.full((n + 2 * GUARD,), 7.0, dtype=torch.float32, device=answers.device)
    idx = torch.full((n + 2 * GUARD,), 7, dtype=torch.int32, device=answers.device)
    rc = lib.pv_neuron_attribution_topk(*args, k, by, val[GUARD:].data_ptr(), idx[GUARD:].data_ptr(), ws.data_ptr(), need,
                                        torch.cuda.current_stream().cuda_stream)
    assert rc == expect, _native.last_error()
    torch.cuda.synchronize()
    shape = (B, t_out, O, max(k, 1))
    return val, idx, val[GUARD:GUARD + n].view(shape), idx[GUARD:GUARD + n].view(shape)


@functools.lru_cache(maxsize=None)
def device_inputs(shape, per_image):
    case = NC.make_case(shape, per_image)
    L = case.post.shape[0]
    post = [torch.from_numpy(case.post[l]).cuda().to(torch.bfloat16).contiguous() for l in range(L)]
    W_out = [torch.from_numpy(case.W_out[l]).cuda().to(torch.bfloat16).contiguous() for l in range(L)]
    return case, post, W_out, torch.from_numpy(case.scale).cuda(), torch.from_numpy(case.answers).cuda()


DENSE_CASES = [(shape, per_image, pos) for shape in NC.SHAPES for per_image in (False, True) for pos in (-1, 0, shape[1] - 1)]


def case_id(c) -> str:
    return f"{NC.shape_id(c[0])}-{'per-image' if c[1] else 'shared'}-pos{c[2]}"


@pytest.mark.parametrize("shape,per_image,pos", DENSE_CASES, ids=[case_id(c) for c in DENSE_CASES])
def test_dense_planted_cases_within_the_derived_bound(shape, per_image, pos):
    case, post, W_out, scale, answers = device_inputs(shape, per_image)
    whole, view = dense(post, W_out, scale, answers, pos=pos)
    assert bool((whole[:GUARD] == 7.0).all()) and bool((whole[-GUARD:] == 7.0).all()), "written outside the output"
    assert not bool((view == 7.0).any()), "an element inside the output was not written"
    got = view.cpu().numpy()
    truth, bound = NC.select_pos(case.truth, pos), NC.select_pos(case.bound, pos)
    nan, zero = NC.select_pos(case.nan, pos), NC.select_pos(case.zero, pos)
    assert got.shape == truth.shape
    assert np.isnan(got[nan]).all(), "a neuron whose post is a NaN or an infinity must be NaN in every column"
    assert np.isfinite(got[~nan]).all(), "a non-finite neuron leaked into another neuron"
    assert (got[zero] == 0).all(), "a neuron whose post is zero must be exactly 0"
    live = ~nan & ~zero
    ratio = np.abs(got[live].astype(np.float64) - truth[live]) / bound[live]
    print(f"{case_id((shape, per_image, pos))}: worst |got - truth| / bound = {ratio.max():.4f}")
    assert ratio.max() <= 1.0
    if pos < 0:
        assert nan.any() and zero.any()
    if per_image:
        ok = ~nan[0]
        assert np.array_equal(got[1][ok], -got[0][ok]), "image 1 (negated answers, the same post) is not the exact negative of image 0"


@functools.lru_cache(maxsize=None)
def dense_and_order(shape, per_image, pos, by):
    """the dense kernel's own output (host, fp32 [B, T_out, L M, O]) and the oracle's order on it up to k = 256"""
    case, post, W_out, scale, answers = device_inputs(shape, per_image)
    _, view = dense(post, W_out, scale, answers, pos=pos)
    got = view.cpu().numpy().copy()
    return got, NC.topk_order(got, min(256, got.shape[2]), by)


TOPK_CASES = [(shape, per_image, -1, min(k, shape[2] * shape[3]), by)
              for shape in NC.SHAPES for per_image in (False, True) for k in (1, 2, 3, 16, 256) for by in (0, 1)]
TOPK_CASES += [(NC.SHAPES[0], per_image, -1, NC.SHAPES[0][2] * NC.SHAPES[0][3], by) for per_image in (False, True) for by in (0, 1)]
TOPK_CASES += [(shape, True, pos, 3, 1) for shape in NC.SHAPES for pos in (0, shape[1] - 1)]


@pytest.mark.parametrize("shape,per_image,pos,k,by", TOPK_CASES, ids=[f"{case_id(c[:3])}-k{c[3]}-by{c[4]}" for c in TOPK_CASES])
def test_topk_equals_the_oracle_on_the_dense_output(shape, per_image, pos, k, by):
    case, post, W_out, scale, answers = device_inputs(shape, per_image)
    B, T, L, M, d, O = shape
    got, order = dense_and_order(shape, per_image, pos, by)
    val_buf, idx_buf, val, idx = topk(post, W_out, scale, answers, k, by, pos=pos)
    for buf in (val_buf, idx_buf):
        assert bool((buf[:GUARD] == 7).all()) and bool((buf[GUARD + val.numel():] == 7).all()), "written outside the output"
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    assert idx.shape == (B, T if pos < 0 else 1, O, k)
    assert idx.min() >= 0 and idx.max() < L * M
    want = order[..., :k]
    assert np.array_equal(idx, want), "the selection or its order differs from the oracle on the dense output"
    dense_at = np.take_along_axis(np.moveaxis(got, -1, -2), want, axis=-1)
    assert np.array_equal(val.view(np.uint32), dense_at.view(np.uint32)), "val does not carry the dense kernel's bits"
    if pos < 0:
        # what the planted tokens are there for (the oracle's answer, which idx equals)
        flat = [l * M + n for l, n in NC.tie_neurons(L, M)]
        if by == 1:
            assert (want[:2, NC.TOK_TIE, :, :min(k, 4)] == np.array(flat[:min(k, 4)])).all()
        if 5 < k <= L * M - 5:
            zeros = dense_at[:, NC.TOK_SPARSE, :, -1]
            assert (zeros == 0).all(), "beyond the five live neurons of the sparse token the k-th entry is a zero of the mass tie"
        nonfinite = sorted(l * M + n for l, n in NC.nonfinite_neurons(L, M))
        assert (want[:, NC.TOK_NONFINITE, :, :min(k, 2)] == np.array(nonfinite[:min(k, 2)])).all()


def test_refusals_launch_nothing():
    case, post, W_out, scale, answers = device_inputs(NC.SHAPES[0], False)

    def untouched(*bufs):
        return all(bool((b == 7).all()) for b in bufs)

    whole, _ = dense(post, W_out, scale, answers, n_answers=17, expect=1)
    assert "16" in _native.last_error() and untouched(whole)
    whole, _ = dense(post, W_out, scale, answers, d_mlp=36, expect=1)
    assert "d_mlp" in _native.last_error() and untouched(whole)
    whole, _ = dense(post, W_out, scale, answers, ws_bytes=64, expect=3)
    assert "workspace" in _native.last_error() and untouched(whole)
    whole, _ = dense(post, W_out, scale, answers, pos=NC.SHAPES[0][1], expect=1)
    assert "pos" in _native.last_error() and untouched(whole)
    for k, by, text in ((0, 0, "PV_NATTR_MAX_K"), (257, 0, "PV_NATTR_MAX_K"), (81, 0, "n_layers * d_mlp"), (3, 2, "by must be")):
        val, idx, _, _ = topk(post, W_out, scale, answers, k, by, expect=1)
        assert text in _native.last_error() and untouched(val, idx)


# ---------------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------------
def float64_spelling(cache, answers, layer, pos):
    """(truth, bound) [B, T_out, layer * d_mlp, O] float64: the composition on float64 copies of the cached mlp.hook_post, the
    model's W_out and the cached scale, and the bound of _neuron_attribution_cases on the same operands"""
    model = cache.model
    n_layers = model.cfg.n_layers
    post = np.stack([cache[f"blocks.{l}.mlp.hook_post"].float().cpu().numpy() for l in range(layer)])
    W_out = np.stack([model.blocks[l].mlp.W_out.detach().float().cpu().numpy() for l in range(layer)])
    key = "ln_final.hook_scale" if layer == n_layers else f"blocks.{layer}.ln1.hook_scale"
    scale = cache[key][..., 0].cpu().numpy()
    truth, bound = NC.truth_and_bound(post, W_out, answers.float().cpu().numpy(), scale)
    return NC.select_pos(truth, -1 if pos is None else pos), NC.select_pos(bound, -1 if pos is None else pos)


def check_end_to_end(cache, d_model, n_images):
    M = cache.model.cfg.d_mlp
    n_layers = cache.model.cfg.n_layers
    gen = torch.Generator().manual_seed(5)
    shared = (0.05 * torch.randn(20, d_model, generator=gen) + 0.02).cuda()              # 20 answers: two chunks
    per_image = (0.05 * torch.randn(n_images, 3, d_model, generator=gen) + 0.02).cuda()
    logit_attribution.use_native(True)
    try:
        for answers, layer, pos in ((shared, None, None), (per_image, None, 0), (shared, 1, 0), (per_image, n_layers, None)):
            with torch.no_grad():
                got, labels = neuron_logit_attribution(cache, answers, layer=layer, pos=pos)
            assert logit_attribution.last_run_native, logit_attribution.native_fallback_reason
            lay = n_layers if layer is None else layer
            assert labels == [f"L{l}N{n}" for l in range(lay) for n in range(M)]
            truth, bound = float64_spelling(cache, answers, lay, pos)
            assert got.dtype == torch.float32 and tuple(got.shape) == truth.shape
            live = bound > 0
            ratio = np.abs(got.cpu().numpy().astype(np.float64) - truth)[live] / bound[live]
            print(f"layer={layer} pos={pos} answers={tuple(answers.shape)}: worst |HIP - float64| / bound = {ratio.max():.4f}")
            assert np.isfinite(ratio).all() and ratio.max() <= 1.0
            assert (got.cpu().numpy()[~live] == 0).all()
            for by, k in (("value", 16), ("abs", 5)):
                with torch.no_grad():
                    top = top_neuron_logit_attribution(cache, answers, k, layer=layer, pos=pos, by=by)
                assert logit_attribution.last_run_native, logit_attribution.native_fallback_reason
                order = NC.topk_order(got.cpu().numpy(), k, int(by == "abs"))
                assert top.layer.dtype == top.neuron.dtype == torch.int64 and top.values.dtype == torch.float32
                assert np.array_equal((top.layer * M + top.neuron).cpu().numpy(), order)
                assert torch.equal(top.values.cpu(), torch.gather(got.cpu().movedim(-2, -1), -1, torch.from_numpy(order)))
            # the PyTorch path of the same call: the same shape and dtype
            logit_attribution.use_native(False)
            with torch.no_grad():
                ref = neuron_logit_attribution(cache, answers, layer=layer, pos=pos, return_labels=False)
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
