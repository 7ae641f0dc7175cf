"""The adversarial attention cases (tests/_attention_cases.py) do what they claim, on the CPU: their float64 reference has the maxima,
regimes and bad rows the GPU tests rely on; a correct kernel passes the checker; each of a list of deliberately wrong kernels fails it.

``twin`` is a CPU statement of the two-pass kernels (attn_lean_kernel / attn_stream_kernel): fp32 arithmetic, scores and pattern
rounded to the storage dtype, 32-key tiles, an online (max, sum) per half-lane -- a lane of the swapped product holds the keys
(e & 3) + 8 (e >> 2) + 4 half of a tile -- merged at the end, NaN rows zeroed per row.  ``mutant`` breaks one thing in it.
"""
import math

import pytest
import torch

import _attention_cases as AC

# every (dtype, d_head, T) of tests/test_attention_adversarial_gpu.py
GPU_T = (17, 50, 64, 65, 257, 626, 677, 1025)
DH = (32, 64)
MUTANTS = ("zero_pattern", "scaled_by_2", "no_max_subtraction", "pad_keys_scored_0", "no_rescale_on_last_tile",
           "halves_merged_without_rescale", "bad_row_zeroes_its_group", "bad_row_left_nan", "head_1_reads_head_0_keys")


def _store(t, dtype):
    return t.to(dtype).to(torch.float32)


def twin(q, k, v, dtype, dh, mutant=None):
    """(scores, pattern [B, H, T, T], z [B, T, H, dh]) as fp32 tensors holding `dtype` values"""
    T = q.shape[1]
    kk = k.clone()
    if mutant == "head_1_reads_head_0_keys":
        kk[:, :, 1] = k[:, :, 0]
    s = _store(torch.einsum("bqhd,bkhd->bhqk", q, kk) / torch.tensor(math.sqrt(dh), dtype=torch.float32), dtype)
    ntile = (T + 31) // 32
    pad = ntile * 32 - T
    sp = torch.cat((s, torch.full(s.shape[:-1] + (pad,), 0.0 if mutant == "pad_keys_scored_0" else float("-inf"))), dim=-1)
    half_of = (torch.arange(32) >> 2) & 1
    m = torch.full(s.shape[:-1] + (2,), float("-inf"))
    l = torch.zeros(s.shape[:-1] + (2,))
    for kt in range(ntile):
        tile = sp[..., 32 * kt:32 * kt + 32]
        for hf in (0, 1):
            sc = tile[..., half_of == hf]
            mn = torch.maximum(m[..., hf], sc.amax(-1))
            part = torch.exp(sc - mn[..., None]).sum(-1)
            keep = torch.ones_like(mn) if (mutant == "no_rescale_on_last_tile" and kt == ntile - 1 and kt > 0) else torch.exp(m[..., hf] - mn)
            l[..., hf] = l[..., hf] * keep + part
            m[..., hf] = mn
    M = m.amax(-1)
    if mutant == "halves_merged_without_rescale":
        L = l.sum(-1)
    else:
        L = (l * torch.exp(m - M[..., None])).sum(-1)
    ok = (L > 0) & (L < float("inf")) & (M > float("-inf")) & (M < float("inf"))
    if mutant == "no_max_subtraction":
        e = torch.exp(s)
        p = e / e.sum(-1, keepdim=True)
        ok = ok & ~torch.isnan(p).any(-1)
    else:
        p = torch.exp(s - M[..., None]) / L[..., None]
    if mutant == "bad_row_zeroes_its_group":
        grp = torch.arange(T) // 32
        for g in range(int(grp.max()) + 1):
            ok[..., grp == g] = ok[..., grp == g].all(-1, keepdim=True)
    if mutant == "bad_row_left_nan":
        p = torch.where(ok[..., None], p, torch.full_like(p, float("nan")))
    else:
        p = torch.where(ok[..., None], p, torch.zeros_like(p))
    if mutant == "zero_pattern":
        p = torch.zeros_like(p)
    if mutant == "scaled_by_2":
        p = 2 * p
    p = _store(p, dtype)
    z = _store(torch.einsum("bhqk,bkhd->bqhd", p, v), dtype)
    return s, p, z


def old_bounds_pass(dtype, q, k, v, s, p, z, dh):
    """what test_dino_gpu.check_attention asserted before the element bound: bf16 2^-8 max|ref| + 1e-6 for scores and z, 2^-8 ABSOLUTE
    for the pattern (against the softmax of the stored scores), z against the stored pattern times v"""
    assert dtype == torch.bfloat16
    s_ref = torch.einsum("bqhd,bkhd->bhqk", q, k) / math.sqrt(dh)
    ok = float((s - s_ref).abs().max()) <= AC.BF16_EPS * float(s_ref.abs().max()) + 1e-6
    ok &= float((p - torch.softmax(s, dim=-1)).abs().max()) <= AC.BF16_EPS
    z_ref = torch.einsum("bhqk,bkhd->bqhd", p, v)
    ok &= float((z - z_ref).abs().max()) <= AC.BF16_EPS * float(z_ref.abs().max()) + 1e-6
    return ok


@pytest.fixture(scope="module")
def cases():
    memo = {}

    def get(name, T, dh):
        if (name, T, dh) not in memo:
            memo[name, T, dh] = AC.make_case(name, T, dh)
        return memo[name, T, dh]
    return get


@pytest.mark.parametrize("dh", DH)
@pytest.mark.parametrize("T", GPU_T)
@pytest.mark.parametrize("name", AC.CASES + ("benign",))
def test_values_are_bf16_and_heads_differ(cases, name, T, dh):
    q, k, v = cases(name, T, dh)
    for t in (q, k, v):
        assert t.shape == (AC.B, T, AC.H, dh) and t.dtype == torch.float32
        same = (t == t.to(torch.bfloat16).float()) | torch.isnan(t)
        assert bool(same.all())
    assert bool(torch.isfinite(v).all())
    s = AC.reference_scores(q, k, dh)
    flat = torch.nan_to_num(s, nan=0.0, posinf=0.0, neginf=0.0).reshape(AC.B * AC.H, -1)
    for a in range(AC.B * AC.H):
        for b in range(a):
            assert not torch.equal(flat[a], flat[b])


@pytest.mark.parametrize("dh", DH)
@pytest.mark.parametrize("T", GPU_T)
def test_peaked_and_shifted_put_the_maxima_where_the_tiles_break(cases, T, dh):
    ntile = (T + 31) // 32
    for name, spread_cap, lo, hi in (("peaked", 80.0, 0.0, 80.0), ("shifted", 10.0, 1024.0, 1024.0)):
        q, k, v = cases(name, T, dh)
        s = AC.reference_scores(q, k, dh)
        assert bool(torch.isfinite(s).all())
        spread = s.amax(-1) - s.amin(-1)
        assert float(spread.max()) <= spread_cap and float(s.abs().max()) <= max(lo, hi)
        if name == "shifted":
            assert float(s[:, :, 0::2].min()) > 980 and float(s[:, :, 1::2].max()) < -980
            assert float(spread.max()) > 8
        else:
            assert float(spread.max()) > 64
        arg = s.argmax(-1)                                                   # [B, H, T]
        strong = torch.arange(T) % 4 == 3                                    # the rows of the largest gain
        # ascending ramp: the running tile maximum rises in EVERY tile, for every strong row, and ends in the ragged last tile
        tiles = torch.nn.functional.pad(s[0, 0][strong], (0, ntile * 32 - T), value=float("-inf")).reshape(-1, ntile, 32).amax(-1)
        assert bool((tiles[:, 1:] > tiles[:, :-1]).all())
        assert bool((arg[0, 0][strong] == T - 1).all()) and T - 1 >= (ntile - 1) * 32
        # descending ramp: key 0
        assert bool((arg[0, 1][strong] == 0).all())
        # spikes: every spike is some strong row's maximum -- the first tile, both sides of each tile edge, the last tile
        hit = set(arg[1, 0][strong].tolist())
        assert hit == set(AC.spike_keys(T))
        if T > 64:
            assert {0, 31, 32, 63, 64, T - 2, T - 1} == hit
        # plateau: equal maxima on both sides of a tile edge
        pl = AC.plateau_keys(T)
        row = s[1, 1][strong][0]
        top = row.max()
        assert bool((row[pl] > top - 0.2).all()) and bool((row[[j for j in range(T) if j not in pl]] < top - 4).all())
        if T >= 36:
            assert pl[0] < 32 <= pl[-1]
        # near-uniform and one-hot rows inside one group of 32 queries (peaked), in every head's first group
        if name == "peaked":
            p = AC.reference_pattern(s)
            pmax = p.amax(-1)
            grp = pmax[1, 0, :min(32, T)]
            assert bool((grp >= 0.99).any()) and bool((grp <= 4.0 / T).any())
            for b in range(AC.B):
                for h in range(AC.H):
                    assert bool((pmax[b, h, :min(32, T)] <= 4.0 / T).any())


@pytest.mark.parametrize("dh", DH)
@pytest.mark.parametrize("T", GPU_T)
def test_nonfinite_has_exactly_the_intended_bad_rows(cases, T, dh):
    q, k, v = cases("nonfinite", T, dh)
    s = AC.reference_scores(q, k, dh)
    p = torch.softmax(s, dim=-1)
    bad = torch.isnan(p).any(-1)                                             # [B, H, T]
    assert bool((torch.isnan(p).all(-1) == bad).all())                       # a row is NaN throughout or nowhere
    want = AC.bad_rows(T)
    for (b, h), rows in want.items():
        assert torch.nonzero(bad[b, h]).flatten().tolist() == rows, (b, h)
    nan_q, pinf_q, ninf_q = want[(0, 0)]
    assert bool(torch.isnan(s[0, 0, nan_q]).all())
    assert bool((s[0, 0, pinf_q] == float("inf")).all()) and bool((s[0, 0, ninf_q] == float("-inf")).all())
    mixed = s[1, 0, T - 1]
    assert bool((mixed == float("inf")).any()) and bool((mixed == float("-inf")).any()) and bool(torch.isinf(mixed).all())
    # the only NaN scores are the all-NaN query row and the NaN key's column: inf * 0 never arose
    nan_s = torch.isnan(s)
    nan_s[0, 0, nan_q] = False
    nan_s[1, 1, :, T // 2] = False
    assert not bool(nan_s.any())
    # placement: bad rows share their group of 32 with good rows; one sits in the last (partial) 128-query block; (0, 1) is clean
    for r in (nan_q, pinf_q):
        g0 = r // 32 * 32
        assert int(bad[0, 0, g0:g0 + 32].sum()) < min(32, T - g0)
    assert want[(0, 0)][-1] // 128 == (T + 127) // 128 - 1 and not bool(bad[0, 1].any())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("dh", DH)
@pytest.mark.parametrize("T", GPU_T)
@pytest.mark.parametrize("name", AC.CASES)
def test_a_correct_kernel_passes_the_checker(cases, name, T, dh, dtype):
    q, k, v = cases(name, T, dh)
    s, p, z = twin(q, k, v, dtype, dh)
    ratios = AC.check(dtype, q, k, v, s, p, z, dh)
    print(AC.report(f"{name} T={T} dh={dh}", ratios))
    assert AC.passes(dtype, ratios), ratios
    # and so does the plain one-pass form (attn_kernel / attn_wave_kernel): softmax of the stored scores in fp32
    p1 = torch.softmax(s, dim=-1)
    p1 = _store(torch.where(torch.isnan(p1), torch.zeros_like(p1), p1), dtype)
    z1 = _store(torch.einsum("bhqk,bkhd->bqhd", p1, v), dtype)
    ratios = AC.check(dtype, q, k, v, s, p1, z1, dh)
    assert AC.passes(dtype, ratios), ratios


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("mutant", MUTANTS)
def test_a_wrong_kernel_fails_the_checker(cases, mutant, dtype):
    """Each mutant is rejected on at least one case, at a T with a ragged last tile (677 = 21 x 32 + 5) and at T = 65."""
    for T, dh in ((677, 64), (65, 32)):
        failed = []
        for name in AC.CASES:
            q, k, v = cases(name, T, dh)
            ratios = AC.check(dtype, q, k, v, *twin(q, k, v, dtype, dh, mutant), dh)
            print(AC.report(f"{mutant} {name} T={T}", ratios))
            if not AC.passes(dtype, ratios):
                failed.append(name)
        assert failed, (mutant, T)


def test_the_old_absolute_pattern_bound_accepts_a_zero_and_a_doubled_pattern_at_677(cases):
    """On what a randomly initialised ViT produces (``benign``) at T = 677 every pattern element is below 2^-8: the older checks pass
    an all-zero pattern and a pattern and z that are both doubled.  The element bound rejects both on the same input."""
    dh, dtype = 64, torch.bfloat16
    q, k, v = cases("benign", 677, dh)
    assert float(AC.reference_pattern(AC.reference_scores(q, k, dh)).max()) < AC.BF16_EPS / 2
    good = twin(q, k, v, dtype, dh)
    assert old_bounds_pass(dtype, q, k, v, *good, dh) and AC.passes(dtype, AC.check(dtype, q, k, v, *good, dh))
    for mutant in ("zero_pattern", "scaled_by_2"):
        wrong = twin(q, k, v, dtype, dh, mutant)
        assert old_bounds_pass(dtype, q, k, v, *wrong, dh), mutant
        ratios = AC.check(dtype, q, k, v, *wrong, dh)
        assert ratios["pattern"] > 1.0 and not AC.passes(dtype, ratios), (mutant, ratios)
        ok, _ = AC.pattern_elementwise_ok(wrong[1], torch.softmax(wrong[0], dim=-1))
        assert not ok
