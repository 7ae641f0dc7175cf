"""tests/_sae_dense_cases.py against itself, on the CPU: the twin of the dense SAE steps passes the checker in every case and both forms,
every slip of the twin fails it in a named case, the reference alone meets the gate condition, and the preconditions the exact assertions
of ``exact_grid`` rest on hold.  The slip table also says what the suite's earlier criterion -- ``rel_fro < 1e-4`` per tensor on
``synth_sae_batch`` at d_in 64, d_sae 512, 256 tokens -- makes of each slip: that is the gap tests/test_sae_dense_planted_gpu.py closes."""
import functools

import numpy as np
import pytest

import _sae_dense_cases as DC
from vit_prisma_amd.synth import synth_sae_batch, synth_sae_state

from conftest import rel_fro

F32, F64 = np.float32, np.float64

# slip -> the planted case (in the split form) that must catch it, in a quantity the GPU test can read back (f is not one: dH overwrites it)
UNSEEN_ON_THE_GPU = ("f", "f_exact", "f_fresh_bits", "dY_fresh_bits")
CAUGHT_BY = {
    "drop_al_bh": "outlier",                   # (``ragged_random`` too, by 1.4 x the bound: the accumulation term of the bound is a worst case)
    "swap_planes_one_kgroup": "outlier",       # (``exact_grid`` cannot: with every lo half 0 the three products still hold a_hi b_hi)
    "flush_lo_denormals": "outlier",
    "scale_from_first_slot_only": "outlier",
    "stale_max": "shrinking",
    "out2_not_in_max": "gated_gate_larger",
    "k_tail_dropped": "exact_grid",
    "inv_scale_once": "ragged_random",
}
assert set(CAUGHT_BY.values()) <= set(DC.CASES)
# what the earlier criterion makes of each slip (asserted below: the table is evidence, not decoration)
OLD_CRITERION_CATCHES = {
    "drop_al_bh": True,                    # round toward zero gives every lo half its value's sign: 2^-11 of every product, all one way
    "swap_planes_one_kgroup": True,        # the same for 8 of every 32 k (a_hi b_lo lost)
    "flush_lo_denormals": False,           # Gaussian operands have no lo half below 2^-14 that matters
    "scale_from_first_slot_only": False,   # the first 256 entries of a Gaussian tensor hold its maximum to within a factor of 2: no clamp
    "stale_max": False,                    # one scale of data per engine
    "out2_not_in_max": False,              # relu(gate) and feature_acts are of one size at the synthetic init
    "k_tail_dropped": False,               # d_in 64, d_sae 512, 256 tokens: every K is a multiple of 32
    "inv_scale_once": True,
}


def run(c, form, slip=None):
    got = DC.twin(c, form, slip)
    if len(c.xs) > 1:
        got["fresh"] = DC.twin(c, form, None, fresh=True)
    return DC.check(c, form, got)


@pytest.mark.parametrize("form", DC.FORMS)
@pytest.mark.parametrize("name", DC.CASES)
def test_twin_meets_the_bounds(name, form):
    c = DC.case(name)
    ratios, msgs = run(c, form)
    print(f"[dense-cases] twin {name} {form}: {DC.fmt(ratios)}")
    assert DC.passes(ratios), msgs
    expected = set(DC.RELU_QUANTITIES + ("f",) if c.kind == "relu" else DC.GATED_QUANTITIES) | {"gates", "fire_count", "l0"}
    assert expected <= set(ratios), expected - set(ratios)


@functools.lru_cache(maxsize=None)
def old_criterion_case(kind):
    """the shape and data of the suite's whole-tensor tests (LayerNorm applied beforehand: the twin has no LN-in of its own)"""
    d_in, d_sae, n = 64, 512, 256
    P = {k: v.copy() for k, v in synth_sae_state(d_in, d_sae, 0).items()}
    P["W_dec"] /= np.linalg.norm(P["W_dec"].astype(F64), axis=1, keepdims=True).astype(F32)
    x = synth_sae_batch(n, d_in, seed=0).astype(F64)
    x = ((x - x.mean(axis=1, keepdims=True)) / (x.std(axis=1, ddof=1, keepdims=True) + 1e-5)).astype(F32)
    if kind == "gated":
        rs = np.random.RandomState(5)
        P.update(b_gate=(0.01 * rs.standard_normal(d_sae)).astype(F32), r_mag=(0.1 * rs.standard_normal(d_sae)).astype(F32),
                 b_mag=(0.01 * rs.standard_normal(d_sae)).astype(F32))
    return DC.Case("synth_" + kind, kind, P, [x, x.copy()])          # (two steps on one engine, as the multi-step tests run)


def old_criterion_catches(slip):
    kind = "gated" if slip == "out2_not_in_max" else "relu"
    c = old_criterion_case(kind)
    ref = DC.reference(c)
    got = DC.twin(c, "split", slip)
    tensors = ("sae_out", "gW_dec", "gW_enc", "gb_dec") + (("gb_enc",) if kind == "relu" else ("gb_gate", "gb_mag", "gr_mag"))
    worst = max(rel_fro(got[q], ref[q]) for q in tensors)
    worst = max(worst, abs(float(got["loss"]) - ref["loss"]) / abs(ref["loss"]))
    return worst >= 1e-4 or not np.isfinite(worst), worst


def test_every_slip_is_caught_by_a_planted_case_and_few_by_the_whole_tensor_criterion():
    assert set(CAUGHT_BY) == set(DC.SLIPS) == set(OLD_CRITERION_CATCHES)
    assert not old_criterion_catches(None)[0]
    rows = []
    for slip in DC.SLIPS:
        c = DC.case(CAUGHT_BY[slip])
        ratios, msgs = run(c, "split", slip)
        failed = {q: v for q, v in ratios.items() if not v <= 1.0 and q not in UNSEEN_ON_THE_GPU}
        old, worst = old_criterion_catches(slip)
        rows.append((slip, CAUGHT_BY[slip], max(failed.values()) if failed else 0.0, ", ".join(sorted(failed)) or "-", old, worst))
    print("\n[dense-cases] slip                          planted case        worst ratio  rel_fro < 1e-4 on synth_sae_batch (64, 512, 256)")
    for slip, name, w, failed, old, worst in rows:
        print(f"[dense-cases] {slip:29s} {name:19s} {w:11.3g}  {'caught' if old else 'MISSED'} (worst {worst:.2e})   fails: {failed}")
    for slip, name, w, failed, old, worst in rows:
        assert w > 1.0, f"{slip} passes the checker in {name}"
        assert old == OLD_CRITERION_CATCHES[slip], (slip, old, worst)
    assert sum(not r[4] for r in rows) >= 4


@pytest.mark.parametrize("name", DC.CASES)
def test_reference_meets_the_gate_condition(name):
    c = DC.case(name)
    for form in DC.FORMS:
        worst, bad = DC.gate_margins(c, form)
        print(f"[dense-cases] {name} {form}: smallest |pre-activation| / bound = {worst:.3g}")
        assert worst > DC.GATE_MARGIN and not bad.any(), (name, form, worst)


def test_shapes_cross_the_tile_and_split_k_boundaries():
    N, D, Fs = DC.BASE
    assert N > DC.DG_BM and N % DC.DG_BM == 4 and N % 4 == 0 and (N + 2) % 4 != 0
    assert D % DC.DG_KSLAB == 8 and D < DC.DG_BN and Fs % DC.DG_BN == 8 and Fs > 2 * DC.DG_BN and D % 8 == 0 and Fs % 8 == 0
    rg = DC.splitk_ranges(Fs)
    assert rg[3][0] == rg[3][1] and rg[2][1] - rg[2][0] == 72 and sum(b - a for a, b in rg) == Fs
    assert DC.case("ragged_exact_form").n == N + 2
    assert np.array_equal(DC.case("ragged_exact_form").x[:N], DC.case("ragged_random").x)


def test_exact_grid_preconditions():
    """every scaled operand of G1 and G2 fits the hi half (lo == 0); W_dec's rows have norm exactly 1 in fp32 (16 entries of +-1/4); every
    product and every partial sum of hidden_pre, the l1 sum and the decoder product is a multiple of a power of two small enough to be exact
    in fp32 whatever the order"""
    c = DC.case("exact_grid")
    r = DC.reference(c)
    Wd = c.P["W_dec"]
    assert ((Wd != 0).sum(axis=1) == 16).all() and (np.abs(Wd[Wd != 0]) == 0.25).all()
    assert ((Wd.astype(F32) ** 2).sum(axis=1, dtype=F32) == 1).all()
    f32 = r["f"].astype(F32)
    assert np.array_equal(f32.astype(F64), r["f"])
    for t in (c.x, c.P["W_enc"], f32, Wd):
        s = DC.scale_of(np.abs(t).max())[0]
        hi, lo = DC.split16(t, s)
        assert (lo == 0).all() and np.array_equal(hi.astype(F64), t.astype(F64) * s)
    # sums of |terms| on their grids stay below 2^24 grid steps: no partial sum in any order can round
    assert (r["hp0_abs"] * 64).max() < 2 ** 24 and np.array_equal(r["hp0_abs"] * 64, np.round(r["hp0_abs"] * 64))
    assert (r["pre_abs"] * 32).max() < 2 ** 24 and np.array_equal(r["pre_abs"] * 32, np.round(r["pre_abs"] * 32))
    assert r["f"].sum() * 8 < 2 ** 24 and c.l1 == 2.0 ** -7 and not c.P["b_dec"].any()
    assert np.array_equal(r["sae_out"].astype(F32).astype(F64), r["sae_out"])
    got = DC.twin(c, "split")
    assert np.array_equal(got["f"], f32) and np.array_equal(got["sae_out"], r["sae_out"].astype(F32))


def test_planted_ranges_are_what_the_cases_claim():
    o, base = DC.case("outlier"), DC.case("ragged_random")
    assert o.x[5, 7] == 2.0 ** 14 and o.P["W_enc"][3, 200] == 2.0 ** 11
    assert 2.0 ** 14 / 4 < o.x[5, 7] / np.median(np.abs(base.x)) and 2.0 ** 14 / 4 < 2.0 ** 11 / np.median(np.abs(base.P["W_enc"]))
    # under the outlier's scale ordinary entries land near 1/2: their lo halves are below 2^-12, a large part of them fp16 denormals
    for t in (o.x, o.P["W_enc"]):
        lo = DC.split16(t, DC.scale_of(np.abs(t).max())[0])[1]
        frac = float(((np.abs(lo) < 2.0 ** -14) & (lo != 0)).mean())
        assert frac > 0.3, frac
    nf = DC.reference(DC.case("no_firing"))
    assert not nf["fire"].any() and nf["P"]["b_dec"].any()
    s = DC.case("shrinking")
    assert len(s.xs) == 2 and np.array_equal(s.xs[0], s.xs[1] * F32(4096.0))
    g = DC.reference(DC.case("gated_gate_larger"))
    n = g["n"]
    top_f, top_g = g["f"].max(axis=1), g["pg"].max(axis=1)
    assert (top_g[:n // 2] >= 2.0 ** 12 * top_f[:n // 2]).all() and (top_f[n // 2:] >= 2.0 ** 12 * top_g[n // 2:]).all()
    assert g["pg"].max() > 8 * g["f"].max()                   # a maximum that covers feature_acts alone sends relu(gate) past 65504
    t = DC.case("tail")
    assert t.activation == "tanh-relu" and t.lp_norm == 2.0


def test_rtz16_is_the_fp16_value_toward_zero():
    rs = np.random.RandomState(0)
    v = (rs.standard_normal(20000) * np.exp2(rs.randint(-30, 18, size=20000))).astype(F32)
    v = np.concatenate([v, np.asarray([0.0, 65504.0, 65519.9, 7e4, 1e9, 2.0 ** -24, 2.0 ** -25, -2.0 ** -14, 2.0 ** -14 - 2.0 ** -30], F32)])
    h = DC.rtz16(v)
    with np.errstate(over="ignore"):
        assert np.array_equal(h.astype(np.float16).astype(F32), h)                          # representable
    assert (np.abs(h) <= np.abs(v)).all() and (np.sign(h) * np.sign(v) >= 0).all()
    inside = np.abs(v) <= 65504
    with np.errstate(over="ignore"):
        up = np.abs(np.nextafter(h.astype(np.float16), np.float16(np.inf) * np.where(v < 0, -1, 1).astype(np.float16)).astype(F32))
    assert (np.abs(v[inside]) < up[inside]).all()                                           # the next fp16 away from zero is beyond v
    assert (np.abs(h[~inside]) == 65504).all()
