"""pv_logit_lens (csrc/lens.hip) on the planted inputs of tests/_lens_cases.py, and the Python surface (vit_prisma_amd/logit_lens.py)
on the tiny bf16 ViT and text tower.  Run with ``-m gpu`` on an MI355X.

Kernel level, per shape of _lens_cases.SHAPES (each the smallest at which a distinct piece of the kernel first runs: N 34 = one
ragged 128-row tile, 260 = two 256-row tiles, the second ragged; S 1, 5; O 24 = less than one wave's columns, 264 = a second
N-tile of 8 columns; d 64 = one full-line slab, 96 and 72 = the barrier-then-fetch loop, whole and ragged last slab, 768 = the real
width), ONE call for the directions and one for the top form, shared by the tests below:
  * every finite element within (d + 4) 2^-24 (sum |x a| + |mean| sum |a|) / scale of the float64 truth; NaN / inf rows all NaN
  * every S-slice holds its own tap's result and no other's
  * top_idx / rank exactly those of the directions the kernel itself stored, and the planted winners, ties and label ranks
  * top_logit bit-identical to the stored direction at top_idx
  * nothing written outside [N, S, O], everything inside written
End to end: get_patch_logit_directions / patch_logit_top report the HIP path and agree with the PyTorch path of the same call
within the reference's own bf16 rounding of mean and centred rows, 2^-8 (sum |xc a| + |mean| sum |a|) / scale.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from vit_prisma_amd import _native, logit_lens

import _lens_cases as LC

pytestmark = pytest.mark.gpu

GUARD = 1024                 # elements of 7.0 on both sides of every output
THIN_MARGIN_CAP = 0.05       # share of cells the end-to-end argmax comparison may exclude for a thin margin


def lens(taps, scale, answers, directions=True, top=False, rank_of=-1, expect=0, dtype=_native.PV_DTYPE_BF16, n_stack=None,
         d_model=None):
    """pv_logit_lens on taps [S][N, d] bf16, scale [N] fp32, answers [O, d] bf16 (CUDA tensors), into buffers prefilled with 7 that
    carry GUARD elements on both sides: {name: (buffer, view)}"""
    lib = _native.lib()
    S, (N, d), O = len(taps), taps[0].shape, answers.shape[0]
    n_stack = S if n_stack is None else n_stack
    d_model = d if d_model is None else d_model
    dev = answers.device

    def buf(n, dtype, fill):
        whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
        return whole, whole[GUARD:GUARD + n]

    out = {}
    if directions:
        out["directions"] = buf(N * S * O, torch.float32, 7.0)
    if top:
        out["top_idx"] = buf(N * S, torch.int32, -7)
        out["top_logit"] = buf(N * S, torch.float32, 7.0)
        if rank_of >= 0:
            out["rank"] = buf(N * S, torch.int32, -7)
    ptr = lambda k: out[k][1].data_ptr() if k in out else None      # noqa: E731
    ws_bytes = lib.pv_logit_lens_workspace_bytes(N, max(n_stack, 1), d_model, O)
    ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=dev)
    ptrs = (C.c_void_p * max(n_stack, S))(*([t.data_ptr() for t in taps] + [taps[0].data_ptr()] * max(n_stack - S, 0)))
    rc = lib.pv_logit_lens(dtype, ptrs, n_stack, N, d_model, scale.data_ptr(), answers.data_ptr(), O, ptr("directions"),
                           ptr("top_idx"), ptr("top_logit"), rank_of, ptr("rank"), ws.data_ptr(), ws.numel(),
                           torch.cuda.current_stream().cuda_stream)
    assert rc == expect, _native.last_error()
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def run_case(shape):
    """(case, directions [N, S, O] float32 numpy, buffers of the directions call, buffers of the top call)"""
    case = LC.make_case(*shape)
    taps = [torch.from_numpy(case.taps[s]).cuda().to(torch.bfloat16).contiguous() for s in range(case.S)]
    scale = torch.from_numpy(case.scale).cuda()
    answers = torch.from_numpy(case.answers).cuda().to(torch.bfloat16).contiguous()
    d_out = lens(taps, scale, answers, directions=True)
    t_out = lens(taps, scale, answers, directions=False, top=True, rank_of=LC.LABEL)
    got = d_out["directions"][1].view(case.N, case.S, case.O).cpu().numpy()
    return case, got, d_out, t_out


SHAPE_PARAMS = pytest.mark.parametrize("shape", LC.SHAPES, ids=LC.shape_id)


@SHAPE_PARAMS
def test_directions_within_the_derived_bound(shape):
    case, got, _, _ = run_case(shape)
    f = case.finite
    assert np.isnan(got[~f]).all(), "a row with a NaN or an infinity in its tap must be NaN in every column"
    assert np.isfinite(got[f]).all()
    ratio = np.abs(got[f].astype(np.float64) - case.truth[f]) / case.bound[f]
    print(f"{LC.shape_id(shape)}: worst |got - truth| / bound = {ratio.max():.4f}; the constant row: "
          f"{np.abs(got[3]).max():.3e} against a bound of {case.bound[3].min():.3e}")
    assert ratio.max() <= 1.0
    # (the reference's own bf16 centring is not this form: it must sit outside, or the bound would not tell the two apart)
    ref = LC.reference_bf16_centring(case)
    assert (np.abs(ref[f] - case.truth[f]) / case.bound[f]).max() > 8.0


@SHAPE_PARAMS
def test_every_stack_slice_comes_from_its_own_tap(shape):
    case, got, _, _ = run_case(shape)
    f = case.finite
    for s in range(case.S):
        for s2 in range(s + 1, case.S):
            apart = np.abs(got[f, s].astype(np.float64) - got[f, s2]) > case.bound[f, s] + case.bound[f, s2]
            assert apart.mean() > 0.5, f"slices {s} and {s2} hold the same values"
    # (that slice s matches tap s is test_directions_within_the_derived_bound: truth[:, s] is computed from tap s alone)


@SHAPE_PARAMS
def test_top_form(shape):
    case, got, _, t_out = run_case(shape)
    N, S = case.N, case.S
    top_idx = t_out["top_idx"][1].view(N, S).cpu().numpy()
    top_logit = t_out["top_logit"][1].view(N, S).cpu().numpy()
    rank = t_out["rank"][1].view(N, S).cpu().numpy()
    # against the directions the kernel stored: exact
    want_idx, want_rank = LC.top_of(got, LC.LABEL)
    assert np.array_equal(top_idx, want_idx)
    assert np.array_equal(rank, want_rank)
    f = case.finite
    at_top = np.take_along_axis(got, top_idx[..., None].astype(np.int64), axis=-1)[..., 0]
    assert np.array_equal(top_logit[f].view(np.uint32), at_top[f].view(np.uint32)), "top_logit is not the stored direction, bit for bit"
    # non-finite rows: index 0, a NaN logit, rank -1
    assert (top_idx[~f] == 0).all() and np.isnan(top_logit[~f]).all() and (rank[~f] == -1).all()
    # against the plan: winners, the tie between the two N-tiles (column 3, not 259), the label's rank
    planted = case.want_top >= 0
    assert np.array_equal(top_idx[planted], np.repeat(case.want_top[planted][:, None], S, axis=1))
    ties = planted & (case.want_top == LC.TIE_LOW)
    assert ties.any() and (top_idx[ties] == LC.TIE_LOW).all()
    if case.O > LC.TIE_HIGH:
        assert np.array_equal(got[ties][..., LC.TIE_LOW].view(np.uint32), got[ties][..., LC.TIE_HIGH].view(np.uint32))
    ranked = case.want_rank >= 0
    assert ranked.any() and np.array_equal(rank[ranked], np.repeat(case.want_rank[ranked][:, None], S, axis=1))


@SHAPE_PARAMS
def test_nothing_outside_the_outputs_is_written_and_everything_inside_is(shape):
    _, _, d_out, t_out = run_case(shape)
    for name, (whole, view) in {**d_out, **t_out}.items():
        fill = 7.0 if whole.dtype == torch.float32 else -7
        assert bool((whole[:GUARD] == fill).all()) and bool((whole[-GUARD:] == fill).all()), f"{name}: written outside"
        assert not bool((view == fill).any()), f"{name}: an element inside was not written"


def test_directions_and_top_in_one_call_without_a_rank():
    case = LC.make_case(*LC.SHAPES[0])
    taps = [torch.from_numpy(case.taps[s]).cuda().to(torch.bfloat16).contiguous() for s in range(case.S)]
    scale, answers = torch.from_numpy(case.scale).cuda(), torch.from_numpy(case.answers).cuda().to(torch.bfloat16).contiguous()
    both = lens(taps, scale, answers, directions=True, top=True)          # no rank: no label launch
    _, _, _, t_out = run_case(LC.SHAPES[0])
    assert torch.equal(both["top_idx"][1], t_out["top_idx"][1])
    assert torch.equal(both["top_logit"][1].view(torch.int32), t_out["top_logit"][1].view(torch.int32))


def test_refusals_state_their_rule():
    case = LC.make_case(*LC.SHAPES[0])
    taps = [torch.from_numpy(case.taps[s]).cuda().to(torch.bfloat16).contiguous() for s in range(case.S)]
    scale, answers = torch.from_numpy(case.scale).cuda(), torch.from_numpy(case.answers).cuda().to(torch.bfloat16).contiguous()
    lens(taps, scale, answers, dtype=_native.PV_DTYPE_F32, expect=1)
    assert "bf16" in _native.last_error()
    lens(taps, scale, answers, d_model=case.d + 4, expect=1)
    assert "multiple of 8" in _native.last_error()
    lens(taps, scale, answers, n_stack=129, expect=1)
    assert "128" in _native.last_error()
    lens(taps, scale, answers, directions=False, top=False, expect=1)
    assert "no output" in _native.last_error()


# ---------------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------------
def rounding_bound(cache, answers, incl_mid):
    """2^-8 (sum_k |xc_k a_k| + |mean| sum_k |a_k|) / scale per cell [B, T, S, O], float64: the reference's bf16 rounding of the
    mean and of the centred rows"""
    stack = cache.accumulated_resid(layer=-1, incl_mid=incl_mid).double()                  # [S, B, T, d]
    a = answers.to(torch.bfloat16).double()
    mean = stack.mean(dim=-1, keepdim=True)
    scale = cache["ln_final.hook_scale"].double()
    bound = 2.0 ** -8 * ((stack - mean).abs() @ a.abs().T + mean.abs() * a.abs().sum(-1)) / scale
    return bound.permute(1, 2, 0, 3)


def graded_answers(d, n_answers, ratio, seed, device):
    """Seeded Gaussian answer rows whose norms grow by `ratio` from row to row: the lead of the top column is then a lead between
    rows of different size, not between two equals.  Shapes and seeds were chosen on the CPU (the PyTorch path on the CPU cache of
    the same model) so that the share of thin-margin cells stays under THIN_MARGIN_CAP: 0.0 % for the ViT (10 rows, ratio 3,
    seed 4), 2.6 % for the text tower (8 rows, ratio 5, seed 16; its floor over 40 seeds -- a row whose projection on the largest
    answer is within the rounding bound of zero is thin whatever the rest)."""
    gen = torch.Generator().manual_seed(seed)
    a = torch.randn(n_answers, d, generator=gen) * (ratio ** torch.arange(n_answers, dtype=torch.float32))[:, None] * 0.01
    return a.to(torch.bfloat16).to(device)


def check_end_to_end(cache, answers, incl_mid, rank_index):
    """The HIP path against the PyTorch path of the same calls; returns the share of cells excluded from the argmax comparison."""
    logit_lens.use_native(True)
    try:
        with torch.no_grad():
            got, labels = logit_lens.get_patch_logit_directions(cache, answers, incl_mid=incl_mid)
            assert logit_lens.last_run_native, logit_lens.native_fallback_reason
            top_idx, top_logit, rank, labels2 = logit_lens.patch_logit_top(cache, answers, incl_mid=incl_mid, rank_index=rank_index)
            assert logit_lens.last_run_native, logit_lens.native_fallback_reason
            table = logit_lens.patch_logit_dictionary(cache, answers, batch_idx=1, incl_mid=incl_mid, rank_label=rank_index)
            assert logit_lens.last_run_native, logit_lens.native_fallback_reason
        logit_lens.use_native(False)
        with torch.no_grad():
            want, want_labels = logit_lens.get_patch_logit_directions(cache, answers, incl_mid=incl_mid)
            assert not logit_lens.last_run_native
            want_idx, _, _, _ = logit_lens.patch_logit_top(cache, answers, incl_mid=incl_mid, rank_index=rank_index)
    finally:
        logit_lens.use_native(None)
    torch.cuda.synchronize()
    assert labels == want_labels == labels2 and got.shape == want.shape and got.dtype == want.dtype == torch.float32
    bound = rounding_bound(cache, answers, incl_mid)
    ratio = ((got.double() - want.double()).abs() / bound).max().item()
    print(f"incl_mid={incl_mid}: worst |HIP - PyTorch| / bound = {ratio:.3f}")
    assert ratio <= 1.0
    # the top form says what the directions say, and the dictionary what the top form says
    mine_idx, mine_rank = LC.top_of(got.cpu().numpy(), rank_index)
    assert np.array_equal(top_idx.cpu().numpy(), mine_idx) and np.array_equal(rank.cpu().numpy(), mine_rank)
    assert torch.equal(top_logit, got.gather(-1, top_idx[..., None])[..., 0])
    T, S = got.shape[1], got.shape[2]
    assert [[cell[2] for cell in table[t]] for t in range(T)] == top_idx[1].tolist()
    assert [[cell[3] for cell in table[t]] for t in range(T)] == rank[1].tolist()
    # argmax against the PyTorch path wherever no other column can cross: both paths are within `bound` of each other per cell, so
    # the top column keeps its place where its lead over every other column exceeds the two cells' bounds together (at most twice
    # the larger of them)
    w = want.double()
    top = w.argmax(dim=-1, keepdim=True)
    lead = w.gather(-1, top) - w
    safe = lead > bound.gather(-1, top) + bound
    safe.scatter_(-1, top, True)
    decided = safe.all(dim=-1)
    excluded = 1.0 - decided.double().mean().item()
    print(f"incl_mid={incl_mid}: {100 * excluded:.2f} % of the cells excluded for a thin margin")
    assert torch.equal(top_idx[decided], want_idx[decided])
    return excluded


@pytest.mark.parametrize("incl_mid", [False, True])
def test_tiny_vit_end_to_end(incl_mid):
    from test_native_vit_gpu import build, run
    from vit_prisma_amd.synth import synth_images
    model, arch, _ = build("tiny", torch.bfloat16)
    _, cache = run(model, synth_images(arch, 2, 1), torch.bfloat16)
    answers = graded_answers(arch["d_model"], 10, 3.0, 4, "cuda")
    assert check_end_to_end(cache, answers, incl_mid, rank_index=5) <= THIN_MARGIN_CAP


def test_tiny_text_tower_end_to_end():
    from test_text_tower_cpu import BATCH, tiny_text_model
    from vit_prisma_amd.synth import ARCHS, synth_tokens
    model = tiny_text_model(torch.bfloat16, "cuda").use_native(True)
    with torch.no_grad():
        _, cache = model.run_with_cache(torch.from_numpy(synth_tokens(ARCHS["tiny-text"], BATCH, seed=1)).cuda())
    assert model.last_run_native, model.native_fallback_reason
    answers = graded_answers(ARCHS["tiny-text"]["d_model"], 8, 5.0, 16, "cuda")
    assert check_end_to_end(cache, answers, True, rank_index=5) <= THIN_MARGIN_CAP
