"""CPU proofs for tests/_sae_apply_cases.py: the planted states hold the classes, ranges, ties and magnitudes they claim; the float64
reference equals oracle/sae_oracle.py's own clip -> project -> Adam on oracle-made gradients; a float32 twin of the kernels' structure
passes every case with its worst error / bound ratio <= 1; eighteen wrong twins -- one per slip the optimizer step could make -- fail on a
named case with a message naming the row; and for each slip, whether the suite's ``rel_fro < 1e-4`` (``2e-4`` for v) on the two random
(64, 512, 8, 256) steps would have seen it."""
import math

import numpy as np
import pytest

import _sae_apply_cases as AC
from oracle import sae_oracle as O
from vit_prisma_amd.synth import synth_sae_batch, synth_sae_state

from conftest import rel_fro

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------ the cases are what they claim
@pytest.mark.parametrize("d_in", AC.WIDTHS)
def test_every_row_class_sits_in_a_full_and_in_the_ragged_tile(d_in):
    c = AC.make(d_in, "active", 2)
    assert (c.d_sae, c.d_in) == (72, d_in) and c.d_sae % 32 == 8 and c.d_sae % 4 == 0
    for k, name in enumerate(AC.ROW_CLASSES):
        rows = np.flatnonzero(c.cls == k)
        assert (rows < 64).any() and (rows >= 64).any(), name
        for lo, hi in ((0, 40), (40, 72), (0, 41), (41, 72)):                   # ... and in every sub-range the GPU tests apply
            assert ((rows >= lo) & (rows < hi)).any(), (name, lo, hi)
    G, M, V, P = c.G, c.M, c.V, c.P
    z, lv, fs = c.cls == AC.ZERO, c.cls == AC.LIVE, c.cls == AC.FIRST
    for key in ("W_encT", "W_dec"):
        assert not G[key][z].any() and not M[key][z].any() and not V[key][z].any()
        assert not G[key][lv].any() and (M[key][lv] != 0).all() and (V[key][lv] > 0).all()
        assert not M[key][fs].any() and not V[key][fs].any()
        e = np.log2(np.abs(G[key][fs].astype(F64)))
        assert e.min() >= -20 and e.max() <= 10 and e.min() < -18 and e.max() > 8
        assert (M[key].astype(F64) ** 2 <= V[key].astype(F64)).all(), key
    for key in c.P:
        assert (M[key].astype(F64) ** 2 <= V[key].astype(F64)).all() and (V[key] >= 0).all(), key
    # orthogonal: the fp32 dot is exactly 0, in the kernels' order and in numpy's
    orth = np.flatnonzero(c.cls == AC.ORTH)
    assert not AC._lane_dot(G["W_dec"][orth], P["W_dec"][orth], AC.v4_of(d_in)).any()
    assert not (G["W_dec"][orth].astype(F64) * P["W_dec"][orth].astype(F64)).sum(axis=1).any()
    # parallel: g = c w
    par = np.flatnonzero(c.cls == AC.PARALLEL)
    ratio = G["W_dec"][par].astype(F64) / P["W_dec"][par].astype(F64)
    assert (np.abs(ratio / ratio[:, :1] - 1) < 4 * AC.U).all()
    # one-hot rows: one element, in the last valid column (both tile kinds) and on every vector boundary below d_in
    hot = np.flatnonzero(c.cls == AC.ONEHOT)
    assert all(np.count_nonzero(G[key][j]) == 1 for j in hot for key in ("W_encT", "W_dec"))
    want = {b for i in range(1, 5) for b in (256 * i - 1, 256 * i) if b < d_in - 1}
    for key, but in (("W_encT", 1024), ("W_dec", 255)):
        cols = [int(np.flatnonzero(G[key][j])[0]) for j in hot]
        assert cols[0] == cols[-1] == d_in - 1 and hot[0] < 64 <= hot[-1]
        assert (want if len(want) <= 7 else want - {but}) <= set(cols), (key, want, cols)


@pytest.mark.parametrize("clip", sorted(AC.CLIPS))
@pytest.mark.parametrize("step", AC.STEPS)
def test_clip_settings_and_the_eps_regime_are_what_they_claim(clip, step):
    c = AC.make(100, clip, step)
    ref = AC.reference(c)
    coef = ref["coef"]
    want = {"disabled": 1.0, "inactive": 1.0, "zero_sq": 1.0}.get(clip)
    if want is not None:
        assert coef == want and ref["coef_err"] == 0.0
    elif clip == "active":
        assert 0.9 * 2.0 ** -7 < coef < 1.1 * 2.0 ** -7
    else:
        assert abs(coef - 0.5) < 1e-6 and float(c.max_grad_norm) == float(F32(1e-6))
        assert abs(math.sqrt(float(c.sq)) - 1e-6) < 1e-13                       # without the + 1e-6 the coefficient would be 1
    bc2 = 1.0 - AC.B2 ** step
    for key, rows in (("W_encT", c.cls == AC.EPSR), ("b_enc", c.cls == AC.EPSR), ("b_dec", np.arange(100) % 8 == AC.EPSR), ("W_dec", c.cls == AC.EPSR)):
        s = np.sqrt(ref["v_" + key][rows] / bc2) / 1e-8
        slack = 3.0 if key != "W_dec" else 3.5                                  # (the projection moves a W_dec row's g~ a little)
        assert s.min() >= 2.0 ** -slack and s.max() <= 2.0 ** slack, (key, s.min(), s.max())
    AC.assert_magnitudes(c, ref)


@pytest.mark.parametrize("d_in,clip,step", AC.COVER)
def test_magnitudes_stay_between_2_to_the_minus_100_and_2_to_the_100(d_in, clip, step):
    for kw in (dict(), dict(pending=True), dict(big=True)):
        AC.assert_magnitudes(AC.make(d_in, clip, step, **kw))


def test_cover_holds_every_width_clip_and_step():
    assert {c[0] for c in AC.COVER} == set(AC.WIDTHS) and {c[1] for c in AC.COVER} == set(AC.CLIPS) and {c[2] for c in AC.COVER} == set(AC.STEPS)
    assert {cl for d, cl, _ in AC.COVER if d == 100} == set(AC.CLIPS) and {s for d, _, s in AC.COVER if d == 260} == set(AC.STEPS)
    assert [AC.v4_of(d) for d in AC.WIDTHS] == [1, 1, 1, 3, 3, 4, 4, 5, 5] and [AC.dpl_of(d) for d in AC.WIDTHS] == [4, 4, 4, 12, 12, 16, 16, 20, 20]
    assert [d % 64 for d in AC.WIDTHS] == [0, 36, 0, 4, 0, 4, 0, 4, 0]            # where the 64-column walk of the tile form goes ragged


def test_weight_classes_round_the_way_they_claim():
    c = AC.make(100, "inactive", 1)
    W = c.P["W_encT"]
    assert set(AC.WEIGHT_ROWS) == set(np.flatnonzero(c.cls == AC.ZERO).tolist())
    with np.errstate(over="ignore"):
        h = W.astype(np.float16)
    by = {}
    for j, kind in AC.WEIGHT_ROWS.items():
        by.setdefault(kind, []).append(j)
    for j in by["fp16_exact"]:
        assert np.array_equal(h[j].astype(F32), W[j])
    for j in by["ties"]:                                                       # 1 + 2^-11 -> 1 (even), 1 + 3 2^-11 -> 1 + 2^-9 (even)
        assert np.array_equal(np.abs(h[j]).astype(F64), np.where(np.arange(100) % 2 == 0, 1.0, 1.0 + 2.0 ** -9))
    for j in by["subnormals"]:
        a = np.abs(W[j].astype(F64)) * 2.0 ** 24
        assert a.max() < 1024 and (a % 1 == 0.5).any() and (a % 1 == 0).any()
        assert np.array_equal(np.abs(h[j]).astype(F64) * 2.0 ** 24, np.where(a % 1 == 0.5, 2 * np.round(a / 2), a))      # ties to even
    for j in by["tiny"]:
        assert np.array_equal(np.abs(h[j]).astype(F64), np.where(np.arange(100) % 3 == 0, 2.0 ** -24, 0.0))              # 2^-25 ties to zero
    for j in by["largest_not_big"]:
        assert W[j, 99] == 60000.0 and W[j, 0] == -60000.0 and not AC.big_rows(W)[j]
    b = AC.make(100, "inactive", 1, big=True)
    assert sorted(b.big) == sorted(AC.BIG_ROWS) and np.array_equal(np.flatnonzero(AC.big_rows(b.P["W_encT"])), sorted(AC.BIG_ROWS))
    assert len({(j // 32, j % 8) for j in b.big}) == len(b.big)                 # no two share a thread of the tile form
    assert {col for col, _ in b.big.values()} == {99, 0, 50}
    with np.errstate(over="ignore", invalid="ignore"):
        hb = b.P["W_encT"].astype(np.float16)
    assert np.isinf(hb[47, b.big[47][0]]) and np.isfinite(hb[38, b.big[38][0]]) and hb[13, b.big[13][0]] == 65504.0
    for j in b.big:
        assert not b.G["W_encT"][j].any() and not b.M["W_encT"][j].any() and not b.V["W_encT"][j].any()


def test_the_constants_differ_by_the_stated_ulps():
    assert float(F32(1) - F32(0.9)) == 0.10000002384185791 and abs(AC.K_C1 / AC.U - 4.0) < 1e-6
    assert float(F32(1) - F32(0.999)) == 0.0009999871253967285 and abs(AC.K_C2 / AC.U - 216.0) < 0.1
    assert AC.K_B2 < 0.22 * AC.U and AC.K_EPS < 0.11 * AC.U and AC.K_1EM6 < 0.44 * AC.U


# ------------------------------------------------------------------------------------------------ the reference is the oracle
def _oracle_case(d_in, d_sae, k, n, steps, max_grad_norm, pending=False):
    """the oracle's own train_step in float64, and before its tail the state as a Case"""
    P = {k_: v.astype(F64) for k_, v in synth_sae_state(d_in, d_sae, 0).items()}
    opt = dict(m={k_: np.zeros_like(v) for k_, v in P.items()}, v={k_: np.zeros_like(v) for k_, v in P.items()})
    stats = dict(n_fwd_since_fired=np.zeros(d_sae), act_freq_scores=np.zeros(d_sae))
    for t in range(steps):
        x = synth_sae_batch(n, d_in, seed=t).astype(F64)
        before = {k_: v.copy() for k_, v in P.items()}
        m0, v0 = ({k_: v.copy() for k_, v in opt[q].items()} for q in ("m", "v"))
        Pc = {k_: v.copy() for k_, v in P.items()}
        O.renorm_decoder(Pc)
        g = O.sae_backward(Pc, x, O.sae_forward(Pc, x, k))
        total = O.train_step(P, opt, stats, x, k, lr=1e-3, step=t + 1, max_grad_norm=max_grad_norm)["grad_norm"]
    tr = lambda D_: dict(W_encT=D_["W_enc"].T.copy(), W_dec=D_["W_dec"], b_enc=D_["b_enc"], b_dec=D_["b_dec"])
    start = tr(before if pending else Pc)
    inv = 1.0 / np.linalg.norm(before["W_dec"], axis=1) if pending else None
    return start, tr(g), tr(m0), tr(v0), total, inv, tr(P), tr(opt["m"]), tr(opt["v"]), steps


@pytest.mark.parametrize("max_grad_norm,pending", [(1.0, False), (0.01, False), (None, False), (0.01, True)])
def test_reference_equals_the_oracles_train_step_tail(max_grad_norm, pending):
    P0, G, M0, V0, total, inv, P1, M1, V1, step = _oracle_case(64, 72, 8, 96, 2, max_grad_norm, pending)
    c = AC.Case("oracle", P0, G, M0, V0, total * total, step, 1e-3, max_grad_norm or 0.0, 0, None, inv_norm=inv)      # (float64 throughout)
    ref = AC.reference(c)
    assert (ref["coef"] < 1.0) == (max_grad_norm == 0.01)
    for key in P1:
        assert rel_fro(ref[key], P1[key]) < 1e-12 and rel_fro(ref["m_" + key], M1[key]) < 1e-12 and rel_fro(ref["v_" + key], V1[key]) < 1e-12, key
        assert rel_fro(ref[key] - P0[key], P1[key] - P0[key])< 1e-9, key                    # the UPDATE, not the weight under it


# ------------------------------------------------------------------------------------------------ the right twin passes every case
def _twin_ratios(c, slip=None, lazy=False):
    ref = AC.reference(c)
    return AC.check(c, ref, AC.twin(c, slip=slip, lazy=lazy), form="rows" if lazy else "tile")


def _variants(d_in, clip, step):
    yield AC.make(d_in, clip, step)
    yield AC.make(d_in, clip, step, j_lo=0, j_hi=41)
    yield AC.make(d_in, clip, step, j_lo=40, j_hi=72)
    yield AC.make(d_in, clip, step, big=True)
    yield AC.make(d_in, clip, step, pending=True, j_lo=0, j_hi=40)


@pytest.mark.parametrize("d_in,clip,step", AC.COVER)
def test_twin_passes_the_planted_states(d_in, clip, step):
    worst = {}
    for c in _variants(d_in, clip, step):
        for lazy in (False, True):
            ratios, msgs = _twin_ratios(c, lazy=lazy)
            assert AC.passes(ratios), (c, lazy, msgs)
            if c.big:
                want = sum(1 for j in c.big for i in range(j // 32 * 32, min(j // 32 * 32 + 32, 72)) if i != j and (i - j) % 8 == 0)
                assert ratios["conservative_inf"] == (0 if lazy else want), (c, lazy, ratios["conservative_inf"])
            else:
                assert ratios["conservative_inf"] == 0
            for q, v in ratios.items():
                worst[q] = max(worst.get(q, 0.0), v)
    print(f"[sae-apply-twin] d_in={d_in} clip={clip} step={step}: {AC.fmt(worst)}")


@pytest.mark.parametrize("extras,d_in", [("transcoder", 100), ("gated", 260)])
def test_twin_passes_the_transcoder_and_gated_states(extras, d_in):
    c = AC.make(d_in, "active", 1000, extras=extras)
    ratios, msgs = _twin_ratios(c)
    print(f"[sae-apply-twin] {c.name}: {AC.fmt(ratios)}")
    assert AC.passes(ratios), msgs
    assert (c.P["W_skip"].size == 10000 and 10000 % 256 == 16) if extras == "transcoder" else set(c.P) >= {"b_gate", "r_mag", "b_mag"}


# ------------------------------------------------------------------------------------------------ the wrong twins fail
# slip -> (make() arguments of the case that shows it, lazy, the quantities whose ratio must exceed 1, seen by rel_fro on the random steps)
# The last column is a fact about the suite as it was, asserted below either way.  Those two steps run at d_in = 64, over the full feature
# range, behind an explicit renorm_decoder() (no renorm pending), from zero moments, with weights of magnitude < 1, and nothing reads a
# shadow: the eleven slips about the coefficient, a pending renorm, a sub-range's edges, the ragged transposed write and the shadows change
# nothing there (parameters / m 1.0e-6, v 1.3e-5: the right twin's own figures).  Seen are seven, each because the random steps happen to
# sit on its degenerate form: at d_in = 64 the one vector a lane holds IS the last one (the projection skipped on whole rows; 4 of 64
# columns of m and v left zero: 0.25); step 1's bias correction from step 0 divides by zero; v after step 1 is 1e-9 .. 1e-7, the size of
# eps (0.13); b_dec has 64 elements, under one 256-element block (1.0); one row of 512 whose m, v stay zero (0.011); and a feature that
# fired in step 1 and not in step 2 has a zero gradient row over live moments (m: 5.7e-3).  What rel_fro cannot do is say which row.
WRONG = {
    "coef_without_1e-6": ((100, "tiny", 1000), {}, False, ("W_dec", "W_encT", "b_enc", "b_dec", "m_W_dec", "v_W_encT"), False),
    "coef_left_out_of_the_dot": ((100, "active", 2), {}, False, ("W_dec", "m_W_dec", "v_W_dec"), False),
    "dot_with_the_unrenormed_row": ((260, "active", 1), dict(pending=True, j_lo=0, j_hi=40), False, ("W_dec", "m_W_dec", "v_W_dec"), False),
    "projection_skipped_in_the_last_ragged_vector": ((260, "active", 1), {}, False, ("W_dec", "m_W_dec", "v_W_dec"), True),
    "last_valid_vector_not_written": ((100, "inactive", 1), {}, False, ("W_dec", "m_W_dec", "v_W_dec"), True),
    "bias_correction_from_step_minus_1": ((260, "active", 2), {}, False, ("W_dec", "W_encT", "b_enc", "b_dec"), True),
    "eps_inside_the_square_root": ((100, "inactive", 1), {}, False, ("W_dec", "W_encT", "b_enc", "b_dec"), True),
    "zero_g_live_moments_rows_skipped": ((64, "disabled", 1), {}, False, ("W_dec", "W_encT", "m_W_dec", "m_W_encT", "v_W_dec", "v_W_encT"), True),
    "row_j_hi_touched": ((100, "active", 2), dict(j_lo=0, j_hi=41), False, ("W_dec", "W_encT", "m_W_encT", "v_W_dec", "W_enc16T", "enc_colsq_outside", "dec_inv_norm_outside"), False),
    "row_j_hi_minus_1_skipped": ((100, "active", 2), dict(j_lo=0, j_hi=40), False, ("W_dec", "W_encT", "m_W_encT", "v_W_dec"), True),
    "b_enc_range_taken_from_0": ((100, "active", 2), dict(j_lo=40, j_hi=72), False, ("b_enc", "m_b_enc", "v_b_enc"), False),
    "W_enc16T_from_the_old_weight": ((64, "disabled", 1), {}, False, ("W_enc16T",), False),
    "enc_colsq_from_the_old_weight": ((1280, "active", 1), {}, False, ("enc_colsq",), False),
    "enc_colsq_without_the_big_rule": ((100, "inactive", 1), dict(big=True), True, ("enc_colsq_big",), False),
    "big_threshold_at_65504": ((100, "inactive", 1), dict(big=True), False, ("enc_colsq_big",), False),
    "transposed_write_drops_the_ragged_rows": ((100, "inactive", 1), {}, False, ("W_enc",), False),
    "dec_inv_norm_from_the_row_before": ((100, "inactive", 1), dict(pending=True), False, ("dec_inv_norm",), False),
    "tail_block_of_a_vector_kernel_dropped": ((100, "active", 1000), dict(extras="transcoder"), False, ("W_skip", "m_W_skip", "v_W_skip", "b_dec", "b_dec_out"), True),
}
assert set(WRONG) == set(AC.SLIPS) and len(WRONG) == 18


def random_steps_rel_fro(slip):
    """The suite's two random (64, 512, 8, 256) steps (test_native_step_vs_oracle: lr 1e-3, max_grad_norm 1, zero moments, an explicit
    renorm before each step) with the oracle's float64 gradient handed to the twin: the worst rel_fro over parameters and first moments,
    the worst over second moments, against the oracle's own float64 train_step."""
    d_in, d_sae, k, n = 64, 512, 8, 256
    P64 = {k_: v.astype(F64) for k_, v in synth_sae_state(d_in, d_sae, 0).items()}
    opt = dict(m={k_: np.zeros_like(v) for k_, v in P64.items()}, v={k_: np.zeros_like(v) for k_, v in P64.items()})
    stats = dict(n_fwd_since_fired=np.zeros(d_sae), act_freq_scores=np.zeros(d_sae))
    tr = lambda D_: dict(W_encT=np.ascontiguousarray(D_["W_enc"].T), W_dec=D_["W_dec"], b_enc=D_["b_enc"], b_dec=D_["b_dec"])
    to32 = lambda D_: {k_: np.ascontiguousarray(v, F32) for k_, v in D_.items()}
    P = to32(tr(P64))
    M = {k_: np.zeros_like(v) for k_, v in P.items()}
    V = {k_: np.zeros_like(v) for k_, v in P.items()}
    worst_pm = worst_v = 0.0
    for t in range(2):
        x = synth_sae_batch(n, d_in, seed=t).astype(F64)
        O.renorm_decoder(P)                                                     # (float32, in place: eng.renorm_decoder())
        Pc = dict(W_enc=P["W_encT"].T.astype(F64), W_dec=P["W_dec"].astype(F64), b_enc=P["b_enc"].astype(F64), b_dec=P["b_dec"].astype(F64))
        g = O.sae_backward(Pc, x, O.sae_forward(Pc, x, k))
        total = O.grad_total_norm(g)
        O.train_step(P64, opt, stats, x, k, lr=1e-3, step=t + 1)
        c = AC.Case("random", P, to32(tr(g)), M, V, F32(total * total), t + 1, F32(1e-3), F32(1.0), 0, None)
        got = AC.twin(c, slip=slip)
        P = {k_: got[k_] for k_ in P}
        M, V = {k_: got["m_" + k_] for k_ in P}, {k_: got["v_" + k_] for k_ in P}
        want, wm, wv = tr(P64), tr(opt["m"]), tr(opt["v"])
        for key in P:
            mine = got["W_enc"].T if key == "W_encT" else P[key]                 # (the suite reads the parameter's own layout)
            with np.errstate(invalid="ignore", over="ignore"):
                a, b, v_ = rel_fro(mine, want[key]), rel_fro(M[key], wm[key]), rel_fro(V[key], wv[key])
            worst_pm = max(worst_pm, *(q if math.isfinite(q) else math.inf for q in (a, b)))
            worst_v = max(worst_v, v_ if math.isfinite(v_) else math.inf)
    return worst_pm, worst_v


@pytest.mark.parametrize("slip", AC.SLIPS)
def test_wrong_twin_fails_on_its_planted_case(slip):
    (d_in, clip, step), kw, lazy, must_fail, seen = WRONG[slip]
    c = AC.make(d_in, clip, step, **kw)
    good, _ = _twin_ratios(c, lazy=lazy)
    assert AC.passes(good)
    bad, msgs = _twin_ratios(c, slip=slip, lazy=lazy)
    print(f"[sae-apply-twin] {slip} on {c.name} rows [{c.j_lo}, {c.j_hi}): {AC.fmt({q: v for q, v in bad.items() if v > 1})}")
    assert not AC.passes(bad)
    for q in must_fail:
        assert bad[q] > 1.0, (q, bad[q])
    assert msgs and all("feature row" in m_ or m_.split(":")[0].lstrip("mv_") in ("b_dec", "b_dec_out", "W_skip") for m_ in msgs), msgs
    worst_pm, worst_v = random_steps_rel_fro(slip)
    print(f"[sae-apply-twin] {slip} on the random (64, 512, 8, 256) steps: worst rel_fro parameters / m {worst_pm:.3g}, v {worst_v:.3g}")
    assert (worst_pm >= 1e-4 or worst_v >= 2e-4) == seen, (slip, worst_pm, worst_v)


def test_the_right_twin_passes_the_random_steps():
    worst_pm, worst_v = random_steps_rel_fro(None)
    print(f"[sae-apply-twin] the right twin on the random steps: worst rel_fro parameters / m {worst_pm:.3g}, v {worst_v:.3g}")
    assert worst_pm < 1e-5 and worst_v < 2e-5
