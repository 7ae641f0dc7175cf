"""The filtered top-k / ReLU encoder of csrc/sae_enc.hip on planted rows (tests/_sae_encoder_cases.py): ``encode_topk`` (listed fallback),
``step`` (folded pre-pass, inline fallback: sae_select_kernel<., true>), ``relu_step``, both forms of the sample pass.  Index sets are the
float64 reference's, every kept value is within a bound assembled from the re-scoring chain; on grid rows the values and the order of a
decided token are the twin's bit for bit and ``fallback_rows()`` is the twin's count of undecided tokens; the filter path and ``sae_exact``
agree; a second call returns the same bits.  Every test prints its worst error / bound."""
import copy

import numpy as np
import pytest
import torch

import _sae_encoder_cases as EC
from vit_prisma_amd.sae.native_sae import NativeSAE

pytestmark = pytest.mark.gpu


def engine(c):
    rs = np.random.RandomState(1)
    W_dec = rs.standard_normal((c.d_sae, c.d_in))
    W_dec = (W_dec / np.linalg.norm(W_dec, axis=1, keepdims=True)).astype(np.float32)
    T = [torch.from_numpy(np.ascontiguousarray(t).copy()).cuda() for t in (c.W, W_dec, c.b, np.zeros(c.d_in, np.float32))]
    eng = NativeSAE(*T, c.k, False, c.n)                            # normalisation off, b_dec = 0: sae_in is x bit for bit
    assert eng.filtered_encoder
    return eng


def bits(t):
    return t.contiguous().view(torch.int32)


def by_index(idx, val):
    o = np.argsort(idx, axis=1, kind="stable")
    return np.take_along_axis(idx, o, 1), np.take_along_axis(val, o, 1)


def verdict(c, label, idx, val, n_fb, tw):
    """the assertions every entry point shares"""
    r = EC.reference(c)
    worst, msgs = EC.check(c, dict(idx=idx, val=val))
    print(f"[encoder-planted] {label}: worst error / bound {worst:.3g}; {n_fb} fallback rows (twin: {tw['fallbacks']})")
    assert worst <= 1, f"{label}: " + "; ".join(msgs[:8])
    undecided = [o != "decided" for o in tw["outcome"]]
    if any(o == "hcap?" for o in tw["outcome"]):                    # which rows are marked depends on wave order
        assert 1 <= n_fb <= sum(undecided), label
    else:
        assert n_fb == tw["fallbacks"], f"{label}: {n_fb} fallback rows, the twin has {tw['fallbacks']}: " + ", ".join(
            sorted({f"{c.labels[n]} -> {tw['outcome'][n]}" for n in range(c.n) if undecided[n]}))
    for n in range(c.n):
        where = f"{label}: token {n} ({c.labels[n]}, twin: {tw['outcome'][n]})"
        if not undecided[n] and c.style == "grid":                  # value descending, index ascending
            assert np.array_equal(idx[n], tw["idx"][n]), f"{where}: order {idx[n].tolist()}, twin {tw['idx'][n].tolist()}"
        if c.style == "grid":
            if not undecided[n] or not r["tie"][n]:
                gi, gv = by_index(idx[n:n + 1], val[n:n + 1])
                ti, tv = by_index(tw["idx"][n:n + 1], tw["val"][n:n + 1])
                assert np.array_equal(gi, ti) and np.array_equal(gv.view(np.uint32), tv.view(np.uint32)), f"{where}: values differ from the twin's bits"
            else:
                assert np.array_equal(np.sort(val[n]).view(np.uint32), np.sort(tw["val"][n]).view(np.uint32)), where


def same_result(c, tw, first, second, label):
    """two runs of one batch: a decided token's list bit for bit and in order; an undecided one's by index (the exact path orders its list
    as its atomics are served), or as a multiset of values where ranks k and k + 1 tie"""
    (idx, val), (idx2, val2) = first, second
    r = EC.reference(c)
    dec = torch.from_numpy(np.asarray([o == "decided" for o in tw["outcome"]])).cuda()
    tie = torch.from_numpy(r["tie"]).cuda()
    assert torch.equal(idx[dec], idx2[dec]) and torch.equal(bits(val[dec]), bits(val2[dec])), f"{label}: decided tokens differ"
    o, o2 = idx.sort(dim=1).indices, idx2.sort(dim=1).indices
    rest = ~dec & ~tie
    assert torch.equal(idx.gather(1, o)[rest], idx2.gather(1, o2)[rest]), f"{label}: undecided tokens differ"
    assert torch.equal(bits(val.gather(1, o)[rest]), bits(val2.gather(1, o2)[rest])), f"{label}: undecided tokens' values differ"
    assert torch.equal(bits(val.sort(dim=1).values), bits(val2.sort(dim=1).values)), f"{label}: values differ"


@pytest.mark.parametrize("name", EC.CASES)
def test_encode_topk_on_planted_rows(name, tuning):
    c, tw = EC.case(name), EC.twin(EC.case(name))
    eng = engine(c)
    x = torch.from_numpy(c.x).cuda()
    idx, val = (t.clone() for t in eng.encode_topk(x)[:2])
    n_fb = eng.fallback_rows()
    idx2, val2 = (t.clone() for t in eng.encode_topk(x)[:2])
    assert eng.fallback_rows() == n_fb or "hcap?" in tw["outcome"]          # (there the marked rows depend on wave order)
    tuning("sae_exact", 1)
    idx_e, val_e = (t.clone() for t in eng.encode_topk(x)[:2])
    tuning("reset")
    torch.cuda.synchronize()
    verdict(c, f"encode_topk {name}", idx.cpu().numpy().astype(np.int64), val.cpu().numpy(), n_fb, tw)
    same_result(c, tw, (idx, val), (idx2, val2), f"{name}: the second call")
    # the exact path: within the bounds on its own, the same sets where there is no tie, and on grid rows the same bits
    worst, msgs = EC.check(c, dict(idx=idx_e.cpu().numpy().astype(np.int64), val=val_e.cpu().numpy()))
    assert worst <= 1, f"{name} sae_exact: " + "; ".join(msgs[:8])
    no_tie = torch.from_numpy(~EC.reference(c)["tie"]).cuda()
    assert torch.equal(idx.sort(dim=1).values[no_tie], idx_e.sort(dim=1).values[no_tie]), f"{name}: filter and exact path disagree"
    if c.style == "grid":
        assert torch.equal(bits(val.sort(dim=1).values), bits(val_e.sort(dim=1).values)), f"{name}: filter and exact path values"


@pytest.mark.parametrize("name", ["edges", "k32", "band_inversion_64"])
def test_step_with_the_inline_fallback_on_planted_rows(name, tuning):
    """``step``: the pre-pass folded into the launches, an undecided token recomputed by its own select workgroup"""
    c, tw = EC.case(name), EC.twin(EC.case(name))
    eng = engine(c)
    x = torch.from_numpy(c.x).cuda()
    tuning("sae_inline_fb", 1)
    out = []
    for _ in range(2):
        eng.step(x)
        torch.cuda.synchronize()
        out.append((eng.topk_idx[:c.n].clone(), eng.topk_val[:c.n].clone(), eng.fallback_rows()))
    tuning("reset")
    (idx, val, n_fb), (idx2, val2, n_fb2) = out
    verdict(c, f"step {name}", idx.cpu().numpy().astype(np.int64), val.cpu().numpy(), n_fb, tw)
    assert n_fb == n_fb2
    same_result(c, tw, (idx, val), (idx2, val2), f"step {name}: the second call")


@pytest.mark.parametrize("name", ["edges", "band_inversion_64", "one_round"])
def test_sample_pass_in_256_row_tiles_and_the_other_k_loops(name, tuning):
    """d_in 64 takes the sample pass in 128-row tiles by default; here the 256-row form, then the barrier-then-fetch and pipelined K loops
    (HCAP is 4096 there, which no planted block of these cases reaches), the per-block epilogue in the full-line loop (``enc_rounds``:
    the case's own HCAP, a compaction round per 32-row block -- ``one_round`` is the planted shape that takes the one-round epilogue by
    default, and the two forms share the wave scan) and the unfused pre-pass (``sae_fold`` 0: sae_wmax_kernel in a launch of its own,
    the filter's form as by default): every form gives the default's bits on decided tokens"""
    c = EC.case(name)
    tw = EC.twin(c)
    other = copy.copy(c)
    other.hcap, other.one_round = 4096, False
    rounds = copy.copy(c)
    rounds.one_round = False
    for form in (other, rounds):
        tw_other = EC.twin(form)
        assert tw_other["outcome"] == tw["outcome"] and "hcap?" not in tw["outcome"]
    eng = engine(c)
    x = torch.from_numpy(c.x).cuda()
    idx0, val0 = (t.clone() for t in eng.encode_topk(x)[:2])
    for key, value in (("enc_tm256", 1), ("gemm_loop", 0), ("gemm_loop", 1), ("enc_rounds", 1), ("sae_fold", 0)):
        tuning(key, value)
        idx, val = (t.clone() for t in eng.encode_topk(x)[:2])
        n_fb = eng.fallback_rows()
        tuning("reset")
        verdict(c, f"encode_topk {name} {key}={value}", idx.cpu().numpy().astype(np.int64), val.cpu().numpy(), n_fb, tw)
        same_result(c, tw, (idx0, val0), (idx, val), f"{name} {key}={value} against the default")


def relu_read(eng, c):
    idx, val, cnt = (t.cpu().numpy() for t in eng.relu_pairs())
    return dict(idx=idx.astype(np.int64), val=val, count=cnt)


def test_relu_step_on_planted_zero_crossings(tuning):
    c = EC.case("relu")
    eng = engine(c)
    cap = c.relu_cap
    # the batch that stays sparse
    tw = EC.twin_relu(c)
    x = torch.from_numpy(c.x).cuda()
    runs = []
    for _ in range(2):
        eng.relu_step(x, 1e-3, cap=cap)
        torch.cuda.synchronize()
        assert int(eng.relu_mode.item()) == tw["mode"] == 0
        runs.append(relu_read(eng, c))
    got = runs[0]
    worst, msgs = EC.check_relu(c, got)
    print(f"[encoder-planted] relu_step: worst error / bound {worst:.3g}")
    assert worst <= 1, "; ".join(msgs[:8])
    for n in range(c.n):
        ti, tv = tw["lists"][n]
        m = int(got["count"][n])
        assert m == ti.size and np.array_equal(got["idx"][n][:m], ti), f"token {n} ({c.labels[n]}): {got['idx'][n][:m].tolist()}, twin {ti.tolist()}"
        if not c.labels[n].endswith("dense row"):
            assert np.array_equal(got["val"][n][:m].view(np.uint32), tv.view(np.uint32)), f"token {n} ({c.labels[n]}): values differ from the twin's bits"
        assert (got["val"][n][m:] == 0).all()
    assert max(got["count"]) == cap
    for q in ("idx", "count"):
        assert np.array_equal(runs[0][q], runs[1][q])
    assert np.array_equal(runs[0]["val"].view(np.uint32), runs[1]["val"].view(np.uint32))
    l0_sparse = float(eng.scalars[2])
    assert np.isclose(l0_sparse, np.mean(got["count"]), rtol=1e-6, atol=0)
    # one token with cap + 1 positives: the step runs dense, l0 is the reference's count of positives
    tw2 = EC.twin_relu(c, which=1)
    eng.relu_step(torch.from_numpy(c.x2).cuda(), 1e-3, cap=cap)
    torch.cuda.synchronize()
    assert int(eng.relu_mode.item()) == tw2["mode"] == 1
    assert np.isclose(float(eng.scalars[2]), EC.reference(c, 1)["positive"].sum(axis=1).mean(), rtol=1e-6, atol=0)
    # the exact path (no filter at all: dense) counts the same positives on the first batch
    tuning("sae_exact", 1)
    eng.relu_step(x, 1e-3, cap=cap)
    torch.cuda.synchronize()
    tuning("reset")
    assert int(eng.relu_mode.item()) == 1 and np.isclose(float(eng.scalars[2]), l0_sparse, rtol=1e-6, atol=0)
