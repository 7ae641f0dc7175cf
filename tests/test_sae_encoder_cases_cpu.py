"""tests/_sae_encoder_cases.py against itself, on the CPU: the twin of the filtered encoder equals the float64 reference on every planted
case, every slip of the twin is caught by a named planted case through something the GPU test reads back (the checker, the count of
fallback rows, or the bits of a decided grid token), the planted conditions hold, and the slip table says what the suite's earlier tests
-- ``fallback_rows() == 0`` and exact index sets on ``synth_sae_batch`` at the shapes of ``_FILTER_SHAPES`` -- make of each slip: that is
the gap tests/test_sae_encoder_planted_gpu.py closes.  (One slip, ``slots_ge``, the emulation does catch on the synthetic data: at
768 -> 24576, k 32 one token of the 1100 has a tile list of exactly ``slots`` hits.  The table records it.)"""
import functools

import numpy as np
import pytest

import _sae_encoder_cases as EC
from vit_prisma_amd.synth import synth_sae_batch, synth_sae_state

F32, F64 = np.float32, np.float64

# test_native_sae_gpu._FILTER_SHAPES (that module needs torch and a GPU to import)
FILTER_SHAPES = [(128, 8192, 16, 600), (768, 24576, 32, 1100), (96, 4096, 64, 257), (104, 4096, 16, 300),
                 (768, 49152, 32, 700), (768, 3072, 32, 900), (128, 2048, 8, 300), (1280, 20480, 32, 500)]
# slip -> the planted case that must catch it, and how the GPU test sees it
CAUGHT_BY = {
    "band_Bn": ("band_inversion_64", "check"),
    "c1_halved": ("band_inversion_1032", "check"),
    "no_sq_check": ("k32", "check"),
    "q_plus_1": ("k32", "count"),
    "kth_no_multiplicity": ("edges", "count"),
    "slots_ge": ("edges", "count"),
    "no_overflow_mark": ("one_round", "check"),
    "rank_no_index_tiebreak": ("edges", "check"),
    "relu_thr_zero": ("relu", "check"),
    "band_rounding_m_only": ("bias_dominated_20", "check"),
}
SYNTH_CATCHES = {s: s == "slots_ge" for s in EC.SLIPS}


def as_got(tw):
    return dict(idx=tw["idx"], val=tw["val"])


def relu_got(tw):
    return dict(idx=[l[0] for l in tw["lists"]], val=[l[1] for l in tw["lists"]], count=[len(l[0]) for l in tw["lists"]])


def seen_by_the_gpu_test(c, slip):
    """the ways tests/test_sae_encoder_planted_gpu.py would notice the slipped twin in place of the kernels"""
    if c.relu_cap:
        w, _ = EC.check_relu(c, relu_got(EC.twin_relu(c, slip)))
        return {"check"} if not w <= 1 else set()
    t0, t1 = EC.twin(c), EC.twin(c, slip)
    how = set()
    if not EC.check(c, as_got(t1))[0] <= 1:
        how.add("check")
    if t0["fallbacks"] != t1["fallbacks"]:
        how.add("count")
    dec = [i for i in range(c.n) if t0["outcome"][i] == "decided" == t1["outcome"][i]]
    if not (np.array_equal(t0["idx"][dec], t1["idx"][dec]) and np.array_equal(t0["val"][dec].view(np.uint32), t1["val"][dec].view(np.uint32))):
        how.add("bits")
    return how


@pytest.mark.parametrize("name", EC.CASES)
def test_twin_equals_the_reference(name):
    c = EC.case(name)
    tw = EC.twin(c)
    worst, msgs = EC.check(c, as_got(tw))
    print(f"[encoder-cases] twin {name}: worst error / bound {worst:.3g}, {tw['fallbacks']} of {c.n} tokens fall back")
    assert worst <= 1, msgs
    r = EC.reference(c)
    # decided tokens: the twin's order is the reference's wherever the float64 values differ
    for n in range(c.n):
        if tw["outcome"][n] == "decided" and not r["tie"][n]:
            assert set(tw["idx"][n].tolist()) == set(r["idx"][n].tolist())
    v = EC.case_values(c)
    if c.style == "grid":
        assert v.grid_a                                            # every filter value is exact in fp32: the twin's are the kernel's
        nz = (c.x != 0).sum(axis=1)
        assert (nz == 2).all() and ((c.W[:, :] != 0).sum(axis=0).max() <= c.d_in)
        for n in (0, c.n - 1):                                     # a feature takes weight from one of a token's two rows only
            rows = np.flatnonzero(c.x[n])
            assert ((c.W[rows] != 0).sum(axis=0) <= 1).all()


def test_relu_twin_equals_the_reference_and_predicts_the_mode():
    c = EC.case("relu")
    for which, mode in ((0, 0), (1, 1)):
        tw = EC.twin_relu(c, which=which)
        worst, msgs = EC.check_relu(c, relu_got(tw), which)
        assert worst <= 1 and tw["mode"] == mode, msgs
        counts = [len(l[0]) for l in tw["lists"]]
        assert max(counts) == c.relu_cap + which                   # exactly cap positives stay sparse, cap + 1 go dense
    assert EC.relu_margin(c) > EC.GATE_MARGIN and EC.relu_margin(c, 1) > EC.GATE_MARGIN
    # the dense row: exact value positive, filter value below -B_n / 2 (listed); the mirror (not listed); exact zero (not listed)
    v, B = EC.case_values(c), EC.twin_relu(c)["B"]
    cols = c.dense_cols
    assert v.ref[3, cols["pos_seen_negative"]] > 0 and v.a[3, cols["pos_seen_negative"]] < -0.5 * B[3]
    assert v.ref[3, cols["neg_seen_positive"]] < 0 and v.a[3, cols["neg_seen_positive"]] > 0.5 * B[3]
    assert (v.ref[:, 304] == 0).all() and (v.a[:, 304] == 0).all()
    assert v.ref[0, 300] > 0 and v.a[0, 300] == 0 and v.ref[0, 301] < 0 and v.a[0, 301] >= -B[0]


@functools.lru_cache(maxsize=None)
def synth(shape):
    """the data of test_filtered_encoder_equals_exact_path (LayerNorm applied beforehand, b_enc x 20) and its exact top-k sets"""
    d_in, d_sae, k, n = shape
    P = synth_sae_state(d_in, d_sae, 0)
    x = synth_sae_batch(n, d_in, seed=5).astype(F64)
    x = ((x - x.mean(axis=1, keepdims=True)) / (x.std(axis=1, ddof=1, keepdims=True) + 1e-5)).astype(F32)
    c = EC.Case("synth", "synth", d_in, d_sae, k, P["W_enc"], 20 * P["b_enc"], x, ["synth_sae_batch"] * n)
    v = EC.values(c, fast=True)
    want = np.sort(np.argpartition(-v.e, k - 1, axis=1)[:, :k], axis=1)
    return c, v, want


def earlier_tests_catch(slip):
    """``n_fb == 0`` and exact index sets, at every shape of _FILTER_SHAPES"""
    for shape in FILTER_SHAPES:
        c, v, want = synth(shape)
        tw = EC.twin(c, slip, v=v)
        if tw["fallbacks"] != 0 or not np.array_equal(np.sort(tw["idx"], axis=1), want):
            return True, shape
    return False, None


def test_every_slip_is_caught_by_a_planted_case_and_not_by_the_synthetic_batches():
    assert set(CAUGHT_BY) == set(EC.SLIPS) == set(SYNTH_CATCHES)
    assert earlier_tests_catch(None) == (False, None)
    rows = []
    for slip in EC.SLIPS:
        name, how = CAUGHT_BY[slip]
        seen = seen_by_the_gpu_test(EC.case(name), slip)
        old, shape = (False, None) if slip == "relu_thr_zero" else earlier_tests_catch(slip)      # (no ReLU filter test on that data at all)
        rows.append((slip, name, how, seen, old, shape))
    print("\n[encoder-cases] slip                     planted case          seen through        synth_sae_batch at _FILTER_SHAPES")
    for slip, name, how, seen, old, shape in rows:
        print(f"[encoder-cases] {slip:24s} {name:21s} {', '.join(sorted(seen)) or '-':19s} {'caught at ' + str(shape) if old else 'MISSED'}")
    for slip, name, how, seen, old, shape in rows:
        assert how in seen, f"{slip} passes in {name}"
        assert old == SYNTH_CATCHES[slip], (slip, shape)
    assert sum(not r[4] for r in rows) >= 9


def test_planted_conditions():
    # band_inversion: loser's filter value minus winner's in (B_n, 2 B_n] for every token, while the exact winner is ahead
    for d_in in (64, 1032):
        c = EC.case(f"band_inversion_{d_in}")
        v, tw = EC.case_values(c), EC.twin(c)
        assert len(c.losers) >= c.k
        d = v.a[:, c.losers].min(axis=1) - v.a[:, c.winners].max(axis=1)
        assert (d > tw["B"]).all() and (d <= 2 * tw["B"]).all(), (d / tw["B"]).min()
        assert (v.ref[:, c.winners].min(axis=1) > v.ref[:, c.losers].max(axis=1)).all()
        assert (np.isin(tw["t"], v.a[:, c.losers])).all() and all(o == "decided" for o in tw["outcome"])
        print(f"[encoder-cases] band_inversion_{d_in}: inversion / B_n in [{(d / tw['B']).min():.4f}, {(d / tw['B']).max():.4f}]")
    assert EC.enc_c1(1032) > EC.enc_c1(64) == F32(1.25e-3)
    # the gap margins: every token that is no tie case
    for name in EC.CASES:
        r = EC.reference(EC.case(name))
        if (~r["tie"]).any():
            assert r["gap"][~r["tie"]].min() > EC.GATE_MARGIN, (name, r["gap"][~r["tie"]].min())
    # exact candidate counts, band populations and outcomes of the count cases
    want = {"edges": {"candidate_counts: 255 candidates": (255, "decided"), "candidate_counts: 256 candidates": (256, "decided"),
                      "candidate_counts: 257 candidates": (257, "decided"), "candidate_counts: 1024 candidates": (1024, "decided"),
                      "slot_edges: 128 hits in tile 2": (128, "decided"), "slot_edges: 129 hits in tile 2": (129, "slots"),
                      "zeros: six positives, every other pre-activation +0.0": (2047, "slots")},
            "one_round": {"slot_edges: 64 hits in tile 15": (64, "decided"), "slot_edges: 65 hits in tile 15": (65, "slots")},
            "k64": {"candidate_counts: 1024 candidates": (1024, "decided"), "candidate_counts: 1025 candidates": (1025, "count"),
                    "candidate_counts: fewer than k candidates": (24, "count")},
            "k32": {"all_in_sample: s_q above t, too few candidates": (None, "count"), "all_in_sample: s_q above t, k candidates": (32, "t<sq"),
                    "sq_gate: t just above the threshold, a top-k feature just below it": (32, "t<sq")}}
    for name, scenes in want.items():
        c = EC.case(name)
        tw = EC.twin(c)
        for label, (ncand, outcome) in scenes.items():
            rows = [n for n in range(c.n) if c.labels[n] == label]
            assert rows, label
            for n in rows:
                assert tw["outcome"][n] == outcome and (ncand is None or tw["ncand"][n] == ncand), (name, label, n, tw["outcome"][n], tw["ncand"][n])
    c = EC.case("edges")
    tw = EC.twin(c)
    for total, outcome in ((192, "decided"), (193, "band")):
        rows = [n for n in range(c.n) if c.labels[n] == f"band_population: {total} within the band"]
        assert rows and all(tw["nr"][n] == total and tw["outcome"][n] == outcome for n in rows)
    for t in (0, 31, 32, 255, 256, 259):
        assert c.labels[t].startswith("tile_edges")
    # hcap: every row stays below its slots, the 256-row tile passes HCAP, the ragged tile does not
    c = EC.case("hcap")
    tw = EC.twin(c)
    assert c.one_round and tw["ncand"].max() == 40 < c.slots and 256 * 40 > c.hcap
    assert tw["outcome"][:256] == ["hcap?"] * 256 and tw["outcome"][256:] == ["decided"] * 4
    # all_in_sample at q == k: decided with t == s_q
    c = EC.case("edges")
    n = c.labels.index("all_in_sample: t == s_q, decided")
    assert tw is not None and EC.twin(c)["t"][n] == EC.twin(c)["sq"][n]
    # one_lane: the three-per-lane subset gives a lower s_q than the whole sample would
    c = EC.case("one_round")
    n = c.labels.index("one_lane: the four largest sampled values in lane 5")
    a = EC.case_values(c).a[n]
    assert EC.twin(c)["sq"][n] < np.sort(a[::16])[-c.q]
    # bias_dominated: t / |s_q|
    for r in (20, 10, 4):
        c = EC.case(f"bias_dominated_{r}")
        tw = EC.twin(c)
        assert ((tw["t"] / np.abs(tw["sq"]) > 2.0 ** r * 0.99) & (tw["t"] / np.abs(tw["sq"]) < 2.0 ** r * 1.04)).all()
        v = EC.case_values(c)
        assert (v.a[:, c.C] < v.a[:, c.eight].min(axis=1)).all() and (v.e[:, c.C] > v.e[:, c.eight].max(axis=1)).all()
    # negative rows
    assert (EC.case_values(EC.case("negative")).ref < 0).all()


def test_shapes_are_the_smallest_the_filter_takes_and_cross_its_boundaries():
    assert EC.N_TOK == 256 + 4 and EC.N_TOK > 2 * 128
    assert (EC.tile_slots(2048, 8), EC.tile_slots(4096, 8), EC.tile_slots(2048, 32), EC.tile_slots(2048, 64)) == (128, 64, 128, 256)
    assert (EC.sample_q(8), EC.sample_q(32), EC.sample_q(64)) == (8, 12, 24)
    assert [EC.loop_form(d) for d in (64, 96, 40, 264, 1032)] == [2, 1, 0, 0, 0]
    assert EC.case("one_round").one_round and not EC.case("edges").one_round
    assert not EC.fast_ok(64, 1792, 8) and not EC.fast_ok(24, 2048, 8) and EC.fast_ok(32, 2048, 8)
    shapes = {(EC.case(n).d_in, EC.case(n).d_sae, EC.case(n).k) for n in EC.CASES}
    assert {(64, 2048, 8), (64, 4096, 8), (96, 2048, 32), (40, 2048, 64), (264, 2048, 8), (1032, 2048, 8)} <= shapes


def test_fl16_is_round_to_nearest_even():
    assert EC.fl16(EC.X_DN) == 1 and EC.fl16(EC.X_UP) == F32(1 + EC.U)
    assert EC.fl16(F32(1 + 0.5 * EC.U)) == 1 and EC.fl16(F32(1 + 1.5 * EC.U)) == F32(1 + 2 * EC.U)
