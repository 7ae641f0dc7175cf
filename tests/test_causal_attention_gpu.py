"""attn_causal_kernel (csrc/attention_causal.hip: attn_stream_body with CAUSAL = true) through the kernel-level entry pv_attention, on
the adversarial q, k, v of tests/_attention_cases.py.  Run with ``-m gpu`` on an MI355X.

Reference (float64, here): scores = q k / attn_scale, then ``+ mask`` literally (-inf where key > query: a masked NaN / +inf becomes
NaN, models/layers/attention.py:262-265 with base_text_transformer.py:188-194); pattern = softmax of the STORED scores, NaN -> 0;
z = stored pattern times v.  Bounds: those of _attention_cases' docstring, nothing new -- bf16 eps = 2^-8 per row (scores, z) / per
element (pattern), fp32 relative L2 1e-4 per row, non-finite positions exact with their sign, rows the reference zeroes exactly zero.
The score bound's row maximum is taken over the keys the row can see.

Shapes: both dtypes x d_head {32, 64} x T in {32 (one full tile, one wave), 77 (CLIP's: three tiles, a ragged last one of 13 keys,
wave 2 partly active, wave 3 idle), 129 (a second query block of one query, its diagonal in a fifth tile)}, B = H = 2.
"""
import ctypes as C
import functools
import math

import pytest
import torch

from vit_prisma_amd import _native

import _attention_cases as AC

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
SHAPES = [(dt, dh, T) for dt in (F32, BF16) for dh in (32, 64) for T in (32, 77, 129)]


def _id(shape):
    dt, dh, T = shape
    return f"{'bf16' if dt == BF16 else 'fp32'}-dh{dh}-T{T}"


def attention(dtype, q, k, v, causal, scores=True, pattern=True, expect=0):
    """pv_attention on q, k, v [B, T, H, dh] (any float dtype; cast to `dtype`): (status, scores | None, pattern | None, z)"""
    lib = _native.lib()
    q, k, v = (t.to(dtype).contiguous() for t in (q, k, v))
    B, T, H, dh = q.shape
    s = torch.full((B, H, T, T), 7.0, dtype=dtype, device=q.device) if scores else None
    p = torch.full((B, H, T, T), 7.0, dtype=dtype, device=q.device) if pattern else None
    z = torch.full((B, T, H, dh), 7.0, dtype=dtype, device=q.device)
    rc = lib.pv_attention(_native.PV_DTYPE_BF16 if dtype == BF16 else _native.PV_DTYPE_F32, q.data_ptr(), k.data_ptr(), v.data_ptr(),
                          B, T, H, dh, math.sqrt(dh), int(causal), s.data_ptr() if scores else None, p.data_ptr() if pattern else None,
                          z.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == expect, _native.last_error()
    torch.cuda.synchronize()
    return rc, s, p, z


@functools.lru_cache(maxsize=None)
def _case(name, T, dh):
    return tuple(t.cuda() for t in AC.make_case(name, T, dh))


def masked_scores_check(dtype, q, k, s_got, dh):
    """worst error / bound of the stored masked scores (inf: a non-finite position that differs)"""
    T = q.shape[1]
    s_ref = AC.reference_scores(q, k, dh)
    above = torch.ones(T, T, dtype=torch.bool, device=q.device).triu(1)
    mask = torch.zeros(T, T, dtype=torch.float64, device=q.device).masked_fill(above, float("-inf"))
    s_ref = s_ref + mask                                            # the add itself: NaN / +inf above the diagonal -> NaN
    s_got = s_got.double()
    fin = torch.isfinite(s_ref)
    same = torch.where(fin, torch.isfinite(s_got), (torch.isnan(s_ref) & torch.isnan(s_got)) | (s_got == s_ref))
    if not bool(same.all()):
        return float("inf")
    ref0, got0 = torch.where(fin, s_ref, torch.zeros_like(s_ref)), torch.where(fin, s_got, torch.zeros_like(s_got))
    if dtype == BF16:
        bound = AC.BF16_EPS * ref0.abs().amax(-1, keepdim=True) + 1e-6
        return AC._ratio((got0 - ref0).abs(), bound.expand_as(ref0))
    return AC._ratio(AC._rel_l2_rows(got0, ref0), torch.full(ref0.shape[:-1], AC.FP32_TOL, dtype=torch.float64, device=q.device))


@pytest.mark.parametrize("name", AC.CASES)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_causal_kernel_on_adversarial_inputs(shape, name):
    dtype, dh, T = shape
    q, k, v = _case(name, T, dh)
    _, s_got, p_got, z_got = attention(dtype, q, k, v, causal=1)
    above = torch.ones(T, T, dtype=torch.bool, device="cuda").triu(1).expand(AC.B, AC.H, T, T)
    # above the diagonal: -inf (NaN where the raw score was NaN / +inf) in the scores, exactly 0 in the pattern
    assert bool((torch.isneginf(s_got[above]) | torch.isnan(s_got[above])).all())
    assert bool((p_got[above] == 0).all())
    if name != "nonfinite":
        assert bool(torch.isneginf(s_got[above]).all()) and bool(torch.isfinite(s_got[~above]).all())
        assert bool((p_got.float().sum(-1) > 0.98).all())                 # every row keeps its diagonal: none is zeroed
    ratios = AC.check(dtype, q, k, v, s_got, p_got, z_got, dh)            # pattern and z: from the STORED scores / pattern
    ratios["scores"] = masked_scores_check(dtype, q, k, s_got, dh)
    line = AC.report(f"causal {_id(shape)} {name}", ratios)
    print(line)
    assert AC.passes(dtype, ratios), line
    if name == "nonfinite":
        # a NaN key in the future still poisons the row (the add, not a select): every row of (1, 1) is zeroed, as without the mask
        assert bool((p_got[1, 1] == 0).all()) and bool((z_got[1, :, 1] == 0).all())
        assert bool(torch.isnan(s_got[1, 1, 0, T // 2]))
        assert bool((p_got[0, 1].float().sum(-1) > 0.98).all())           # (0, 1) has no bad row
    # the same pattern and the same z whichever taps are taken
    _, _, p2, z2 = attention(dtype, q, k, v, causal=1, scores=False)
    _, _, _, z3 = attention(dtype, q, k, v, causal=1, scores=False, pattern=False)
    assert torch.equal(p2, p_got) and torch.equal(z2, z_got) and torch.equal(z3, z_got)


@pytest.mark.parametrize("dtype,dh", [(F32, 32), (F32, 64), (BF16, 32), (BF16, 64)], ids=["fp32-dh32", "fp32-dh64", "bf16-dh32", "bf16-dh64"])
def test_the_future_does_not_leak(dtype, dh):
    """Other finite k and v at the keys > t0 leave the rows <= t0 bit-identical: scores (lower triangle), pattern and z."""
    T = 77
    q, k, v = _case("peaked", T, dh)
    _, s0, p0, z0 = attention(dtype, q, k, v, causal=1)
    g = torch.Generator(device="cuda").manual_seed(3)
    k_alt = AC._bf16(3.0 * torch.randn(k.shape, device="cuda", generator=g) + 1.0)
    v_alt = AC._bf16(5.0 * torch.randn(v.shape, device="cuda", generator=g) - 2.0)
    low = torch.ones(T, T, dtype=torch.bool, device="cuda").tril()
    for t0 in (0, 31, 32, 76):
        k1, v1 = k.clone(), v.clone()
        k1[:, t0 + 1:], v1[:, t0 + 1:] = k_alt[:, t0 + 1:], v_alt[:, t0 + 1:]
        assert t0 == T - 1 or not torch.equal(k1, k)
        _, s1, p1, z1 = attention(dtype, q, k1, v1, causal=1)
        rows = slice(0, t0 + 1)
        seen = low[rows].expand(AC.B, AC.H, -1, -1)
        assert torch.equal(s1[:, :, rows][seen], s0[:, :, rows][seen]), t0
        assert torch.equal(p1[:, :, rows], p0[:, :, rows]) and torch.equal(z1[:, rows], z0[:, rows]), t0
        if t0 < T - 1:
            assert not torch.equal(z1[:, t0 + 1:], z0[:, t0 + 1:]), t0     # (the later rows do see the change)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_causal_zero_is_the_normal_dispatch(dtype):
    """causal = 0 through the same entry: the unmasked kernels, held to the unmasked reference."""
    T, dh = 77, 64
    q, k, v = _case("shifted", T, dh)
    _, s_got, p_got, z_got = attention(dtype, q, k, v, causal=0)
    ratios = AC.check(dtype, q, k, v, s_got, p_got, z_got, dh)
    line = AC.report(f"causal=0 {'bf16' if dtype == BF16 else 'fp32'}", ratios)
    print(line)
    assert AC.passes(dtype, ratios), line
    assert bool(torch.isfinite(s_got).all()) and bool((p_got[:, :, 0, 1:].float().sum(-1) > 0).all())


def test_causal_wide_head_is_refused_with_the_rule():
    q = torch.zeros(1, 77, 2, 80, device="cuda")
    attention(F32, q, q, q, causal=1, expect=1)
    why = _native.last_error()
    assert "causal" in why and "{32, 64}" in why and "2048" in why, why
