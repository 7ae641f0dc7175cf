"""The k-sparse SAE tail on planted firing patterns (tests/_sae_backward_cases.py): ``pv_sae_step`` and ``relu_step`` steered by
construction, ``encode_topk -> tp_partial -> tp_finish`` fed the (idx, val) pairs directly.  Index sets, kept values, firing counts, l0,
the statistics and the rows of empty features are held exactly; every element of every gradient row, the reconstruction and the loss are
held to a bound derived from the float64 reference's own absolute sums (no tensor-wide norm).  Every test prints its worst error / bound
ratios (MEASURED.md: "The k-sparse SAE backward on planted firing patterns")."""
import functools

import numpy as np
import pytest
import torch

import _sae_backward_cases as SC
from vit_prisma_amd.sae.native_sae import NativeSAE

from conftest import rel_fro

pytestmark = pytest.mark.gpu
PLANTED = SC.PATTERNS + ("boundaries_2048",)


@functools.lru_cache(maxsize=None)
def planted_ref(name, l1=0.0):
    """one case and one float64 reference per pattern, shared by the tests (read-only)"""
    c = SC.planted(name)
    return c, SC.reference(c.P, c.x, c.idx, c.val, c.norm, l1=l1)


def engine(c, P=None):
    T = {k_: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k_, v in (P or c.P).items()}
    return NativeSAE(T["W_enc"], T["W_dec"], T["b_enc"], T["b_dec"], c.k, c.norm, c.n)


def bits(t):
    return t.contiguous().view(torch.int32)


def reset_stats(eng):
    eng.act_freq_scores.zero_()
    eng.n_fwd_since_fired.fill_(3.0)


def gathered(eng, c, counts, with_out=True):
    """what the step left, as the checker takes it"""
    n = c.n
    torch.cuda.synchronize()
    sc = eng.scalars.cpu().numpy()
    got = dict(loss=sc[0], l0=sc[2], gW_dec=eng.g["W_dec"].cpu().numpy(), gW_enc=eng.g["W_enc"].cpu().numpy(),
               gb_enc=eng.g["b_enc"].cpu().numpy(), gb_dec=eng.g["b_dec"].cpu().numpy(), fire_count=eng.fire_count.cpu().numpy(),
               act_freq_scores=eng.act_freq_scores.cpu().numpy(), act_freq_scores_ref=counts.astype(np.float32),
               n_fwd_since_fired=eng.n_fwd_since_fired.cpu().numpy(), n_fwd_since_fired_ref=np.where(counts > 0, 0.0, 4.0))
    if with_out:
        got["sae_out"] = eng.sae_out[:n].cpu().numpy()
    return got


def verdict(label, ratios, msgs):
    print(f"[sae-planted] {label}: {SC.fmt(ratios)}")
    assert SC.passes(ratios), f"{label}: " + "; ".join(msgs)


def rolled(c):
    """the case's tokens moved on to the next class's score row: another firing pattern on the same parameters"""
    C = int((np.abs(c.P["W_enc"]).sum(axis=1) > 0).sum())
    x = c.x.copy()
    x[:, :C] = np.roll(c.x[:, :C], 1, axis=1)
    return x


@pytest.mark.parametrize("name", PLANTED)
def test_step_on_planted_classes(name, tuning):
    """pv_sae_step, folded and in single launches, dense and sparse gradients, behind another pattern's step (the second writes over the first's
    rows, and zeroes those it empties), twice on the same input.  Token-range form: every bit reproducible and the two launch forms
    bit-equal.  Count-cut form (``count_cut``): the long lists are summed in the order the selection's atomics drew, so their rows are held
    to the bounds only and whether two runs agree is printed; every other row and output must still be the same bits."""
    c, ref = planted_ref(name)
    n, counts = c.n, ref["counts"]
    assert np.array_equal(counts, c.lengths)
    x, x_first = torch.from_numpy(c.x).cuda(), torch.from_numpy(rolled(c)).cuda()
    ranged = SC.long_ranged(n)
    rep_rows = torch.from_numpy(counts <= SC.BWD_LMAX).cuda()                   # rows whose list is in token order in either form
    kept = {}
    for fold in (1, 0):
        tuning("sae_fold", fold)
        eng = engine(c)
        for sparse in (False, True):
            label = f"step {name} fold={fold} sparse_grads={int(sparse)}"
            eng.flat_g.fill_(float("nan"))
            eng.step(x_first, sparse_grads=sparse)
            if sparse:
                eng.flat_g.fill_(float("nan"))
            reset_stats(eng)
            eng.step(x, want_out=True, sparse_grads=sparse)
            got = gathered(eng, c, counts)
            got.update(idx=eng.topk_idx[:n].cpu().numpy(), val=eng.topk_val[:n].cpu().numpy(), val_ref=c.val)
            ratios, msgs = SC.check(ref, got, poison="sparse" if sparse else "dense")
            if eng.filtered_encoder:
                print(f"[sae-planted] {label}: fallback_rows = {eng.fallback_rows()}")
            verdict(label, ratios, msgs)
            eng.grad_sqnorm(from_step=True)
            torch.cuda.synchronize()
            g = eng.flat_g.double()
            own = float((torch.nan_to_num(g) ** 2).sum())
            assert abs(float(eng.scalars[3]) - own) <= 1e-5 * own, (label, float(eng.scalars[3]), own)
            first = (bits(eng.flat_g).clone(), eng.sae_out[:n].clone(), eng.scalars[:4].clone(), eng.fire_count.clone(),
                     torch.sort(eng.topk_idx[:n], dim=1).values.clone())
            kept[(fold, sparse)] = first
            eng.step(x, want_out=True, sparse_grads=sparse)                      # the same input again
            eng.grad_sqnorm(from_step=True)
            torch.cuda.synchronize()
            again = (bits(eng.flat_g), eng.sae_out[:n], eng.scalars[:4], eng.fire_count, torch.sort(eng.topk_idx[:n], dim=1).values)
            same_bits(label + " run 2 against run 1", first, again, ranged, eng, rep_rows)
    for sparse in (False, True):
        same_bits(f"step {name} sparse_grads={int(sparse)} folded against single launches", kept[(1, sparse)], kept[(0, sparse)], ranged,
                  eng, rep_rows)


def same_bits(label, a, b, ranged, eng, rep_rows, names=("sae_out", "fire_count", "index sets")):
    g_same = torch.equal(a[0], b[0])
    for i, what in zip((1, 3, 4), names):
        assert torch.equal(a[i], b[i]), f"{label}: {what}"
    assert torch.equal(a[2][:3], b[2][:3]), f"{label}: loss / l0"
    if ranged:
        assert g_same and torch.equal(a[2], b[2]), f"{label}: gradient bits differ in the token-range form"
        return
    print(f"[sae-planted] {label}: count-cut form, gradient bits {'equal' if g_same else 'DIFFER'}")
    nW = eng.d_in * eng.d_sae
    for o in (0, nW):                                                          # gW_enc^T, gW_dec: the rows of lists that are sorted
        ra, rb = a[0][o:o + nW].view(eng.d_sae, eng.d_in)[rep_rows], b[0][o:o + nW].view(eng.d_sae, eng.d_in)[rep_rows]
        assert torch.equal(ra, rb), f"{label}: a short list's row changed bits"
    assert torch.equal(a[0][2 * nW:2 * nW + eng.d_sae][rep_rows], b[0][2 * nW:2 * nW + eng.d_sae][rep_rows]), f"{label}: gb_enc of a short list"


@pytest.mark.parametrize("d_in", SC.WIDTHS)
@pytest.mark.parametrize("name", SC.PATTERNS)
def test_tp_finish_on_injected_pairs(name, d_in, tuning):
    """encode_topk -> tp_partial(renorm_decoder=False) -> tp_finish on a one-rank shard with the pairs of the pattern (LayerNorm on, the
    decoder renormed beforehand, update_stats on), folded and in single launches.  A negative value is a hole: it must contribute nothing.
    The two launch forms run the same code behind the decode launch (sae_csr_build with and without ``folded``), the loss included: what
    they leave is compared by ``same_bits`` -- every bit in the token-range form, the short lists' rows and the scalars in the count-cut form."""
    c = SC.injected(name, d_in)
    n = c.n
    eng = engine(c)
    eng.renorm_decoder()
    P = dict(c.P, W_dec=eng.params["W_dec"].cpu().numpy())                     # the rows the kernels read
    ref = SC.reference(P, c.x, c.idx, c.val, c.norm)
    counts = ref["counts"]
    assert np.array_equal(counts, c.lengths) and int((c.val < 0).sum()) == min(5, c.holes)
    x, idx, val = torch.from_numpy(c.x).cuda(), torch.from_numpy(c.idx.copy()).cuda(), torch.from_numpy(c.val.copy()).cuda()
    kept = {}
    for fold in (1, 0):
        tuning("sae_fold", fold)
        eng.encode_topk(x, want_ln_stats=False)
        pre = eng.tp_partial(idx, val, renorm_decoder=False)
        eng.flat_g.fill_(float("nan"))
        reset_stats(eng)
        eng.tp_finish(x, pre, idx, val, update_stats=True)
        got = gathered(eng, c, counts, with_out=False)
        got["partial"] = pre.cpu().numpy()
        ratios, msgs = SC.check(ref, got, poison="dense")
        verdict(f"tp_finish {name} d_in={d_in} fold={fold}", ratios, msgs)
        kept[fold] = (bits(eng.flat_g).clone(), eng.act_freq_scores.clone(), eng.scalars[:3].clone(), eng.fire_count.clone(),
                      eng.n_fwd_since_fired.clone())
    same_bits(f"tp_finish {name} d_in={d_in} folded against single launches", kept[1], kept[0], SC.long_ranged(n), eng,
              torch.from_numpy(counts <= SC.BWD_LMAX).cuda(), names=("act_freq_scores", "fire_count", "n_fwd_since_fired"))


@pytest.mark.parametrize("cap", [8, 12])
def test_relu_step_on_boundaries(cap):
    """The sparse form of the ReLU + L1 step on ``boundaries`` at d_sae 2048 (the form exists from 2048 features on: below, relu_step always
    runs the dense GEMMs): the per-token capacity beyond a token's positive activations becomes holes, the L1 term's l1 / N joins dh of
    every kept pair."""
    l1 = 3e-3
    c, ref = planted_ref("boundaries_2048", l1)
    n, counts = c.n, ref["counts"]
    eng = engine(c)
    eng.flat_g.fill_(float("nan"))
    reset_stats(eng)
    eng.relu_step(torch.from_numpy(c.x).cuda(), l1, renorm_decoder=False, want_out=True, cap=cap)
    assert int(eng.relu_mode.item()) == 0
    idx, val, cnt = (t.cpu().numpy() for t in eng.relu_pairs())
    live = ref["live"]
    assert np.array_equal(cnt, live.sum(axis=1)), "pairs per token"
    for t in range(n):                                                         # the kept sets and values, exactly
        o = np.argsort(idx[t, :cnt[t]])
        ro = np.argsort(c.idx[t][live[t]])
        assert np.array_equal(idx[t, :cnt[t]][o], c.idx[t][live[t]][ro]) and np.array_equal(val[t, :cnt[t]][o], c.val[t][live[t]][ro]), t
    got = gathered(eng, c, counts)
    ratios, msgs = SC.check(ref, got, poison="dense")
    sc = eng.scalars.cpu().numpy()
    l1_ok = abs(sc[4] - ref["l1_loss"]) <= SC.gamma(n * c.k + 4) * ref["l1_loss"] + SC.U * ref["l1_loss"]
    ratios["l1_loss"] = 0.0 if l1_ok else float("inf")
    verdict(f"relu_step boundaries_2048 cap={cap}", ratios, msgs + ([] if l1_ok else [f"l1_loss {sc[4]!r} against {ref['l1_loss']!r}"]))


@pytest.mark.parametrize("name", ["boundaries", "all_long65", "all_long64"])
def test_apply_after_dense_and_sparse_gradient_steps(name):
    """apply behind a dense-gradient and behind a sparse-gradient step of the same pattern: the rows of features empty in a step see g = 0 in
    both engines and must come out as the same bits; everything else as test_sparse_gradient_step_lands_on_the_same_parameters_as_the_dense_one
    holds it."""
    c, ref = planted_ref(name)
    dense, sparse = engine(c), engine(c)
    xs = [torch.from_numpy(c.x).cuda(), torch.from_numpy(rolled(c)).cuda(), torch.from_numpy(c.x).cuda()]
    never = None
    for t, x in enumerate(xs):
        dense.step(x, renorm_decoder=True); dense.grad_sqnorm(from_step=True); dense.apply(1e-3, 1.0)
        sparse.flat_g.fill_(float("nan"))
        sparse.step(x, renorm_decoder=True, sparse_grads=True)
        empty = sparse.fire_count == 0
        assert int(empty.sum()) > 0 and torch.equal(sparse.fire_count, dense.fire_count)
        if t != 1:
            assert np.array_equal(sparse.fire_count.cpu().numpy(), ref["counts"])
        assert bool(torch.isnan(sparse.g["W_dec"][empty]).all()) and bool(torch.isnan(sparse.g["W_enc"][empty]).all())
        assert bool(torch.isfinite(sparse.g["W_dec"][~empty]).all()) and bool(torch.isfinite(sparse.g["b_enc"]).all())
        sparse.grad_sqnorm(from_step=True)
        sparse.apply(1e-3, 1.0)
        torch.cuda.synchronize()
        for i in (0, 3):                                                       # loss, clip norm
            assert abs(float(sparse.scalars[i]) - float(dense.scalars[i])) <= 1e-6 * abs(float(dense.scalars[i])), (t, i)
        for pname in ("W_enc", "W_dec", "b_enc", "b_dec"):
            assert rel_fro(sparse.params[pname].cpu().numpy(), dense.params[pname].cpu().numpy()) < 1e-6, (t, pname)
        assert rel_fro(sparse.flat_m.cpu().numpy(), dense.flat_m.cpu().numpy()) < 1e-5, t
        assert rel_fro(sparse.flat_v.cpu().numpy(), dense.flat_v.cpu().numpy()) < 1e-5, t
        never = empty if never is None else (never & empty)
        assert int(never.sum()) > 0
        for rows in ((empty, never) if t == 0 else (never,)):                  # (step 0 starts from identical states: every empty row)
            assert torch.equal(sparse.params["W_dec"][rows], dense.params["W_dec"][rows]), t
            assert torch.equal(sparse.params["W_enc"][:, rows], dense.params["W_enc"][:, rows]), t
            assert torch.equal(sparse._m["W_dec"][rows], dense._m["W_dec"][rows]) and torch.equal(sparse._v["W_encT"][rows], dense._v["W_encT"][rows]), t
            assert torch.equal(sparse.params["b_enc"][rows], dense.params["b_enc"][rows]), t
        assert bool(torch.isfinite(sparse.flat_m).all()) and bool(torch.isfinite(sparse.flat_v).all())
