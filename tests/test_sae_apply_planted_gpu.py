"""The SAE optimizer step on planted states (tests/_sae_apply_cases.py): ``pv_sae_apply`` -- clip, remove the gradient parallel to the decoder
rows, Adam -- and the three copies of the encoder it keeps in step, all through ``NativeSAE`` built on planted parameters with planted
``flat_g`` / ``flat_m`` / ``flat_v`` / ``scalars[3]`` / ``adam_step``.  Every element of every parameter and moment, enc_colsq and dec_inv_norm is
held to a bound derived from the float64 reference's own magnitudes (no tensor-wide norm); the copies, the ``zero`` rows and everything outside
an applied sub-range are held bit for bit.  Every test prints its worst error / bound ratios under ``[sae-apply]`` (MEASURED.md: "The SAE
optimizer step on planted gradients").

``COVER`` (17 of the 9 x 5 x 4 combinations of width, clip setting and step): every width once with the clips and steps cycling, all five clips
at d_in = 100 (ragged inside the first vector and inside the second 64-column pass), all four steps at d_in = 260 (one live lane in the last
vector), the plan's maximum 1280 with the clip active and in the + 1e-6 regime."""
import numpy as np
import pytest
import torch

import _sae_apply_cases as AC
import _sae_backward_cases as SC
from vit_prisma_amd import _native as N
from vit_prisma_amd.sae.native_sae import NativeSAE

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
GATED = ("b_gate", "r_mag", "b_mag")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def plant(eng, c):
    """the case's gradient, moments, clip norm and step count, written where apply reads them"""
    for key in c.P:
        eng._g[key].copy_(dev(c.G[key]))
        eng._m[key].copy_(dev(c.M[key]))
        eng._v[key].copy_(dev(c.V[key]))
    eng.scalars[3] = float(c.sq)
    eng.adam_step = c.step - 1


def engine(c, lazy=False, planted=True):
    P = c.P
    kw = {}
    if "b_dec_out" in P:
        kw.update(b_dec_out=dev(P["b_dec_out"]), W_skip=dev(P["W_skip"]))
    if "b_gate" in P:
        kw.update(gated={k_: dev(P[k_]) for k_ in GATED})
    eng = NativeSAE(dev(P["W_encT"].T), dev(P["W_dec"]), dev(P["b_enc"]), dev(P["b_dec"]), 8, "none", 64, **kw)
    eng.lazy_w_enc = lazy
    if planted:
        plant(eng, c)
    return eng


def snapshot(eng, c):
    torch.cuda.synchronize()
    out = dict(W_encT=eng.W_encT.cpu().numpy(), W_enc=eng.params["W_enc"].cpu().numpy(), W_enc16T=eng.W_enc16T.cpu().numpy(),
               enc_colsq=eng.enc_colsq.cpu().numpy(), dec_inv_norm=eng.dec_inv_norm.cpu().numpy())
    for key in c.P:
        if key != "W_encT":
            out[key] = eng.params[key].cpu().numpy()
        out["m_" + key], out["v_" + key] = eng._m[key].cpu().numpy(), eng._v[key].cpu().numpy()
    return out


def applied(eng, c, w_enc=True):
    """run the apply of the case; -> what ``check`` takes (the shadows with what they held before)"""
    before = snapshot(eng, c)
    eng.apply(float(c.lr), float(c.max_grad_norm) if float(c.max_grad_norm) > 0 else None, c.j_lo, c.j_hi)
    got = snapshot(eng, c)
    assert eng.adam_step == c.step
    for q in ("W_enc16T", "enc_colsq", "dec_inv_norm"):
        got[q + "_before"] = before[q]
    if not w_enc:
        got["W_enc_stale"] = got.pop("W_enc")
    return got, before


def verdict(label, ratios, msgs):
    print(f"[sae-apply] {label}: {AC.fmt(ratios)}")
    assert AC.passes(ratios), f"{label}: " + "; ".join(msgs)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------------------------------------ apply on planted states
@pytest.mark.parametrize("d_in,clip,step", AC.COVER)
def test_apply_on_planted_states(d_in, clip, step):
    """the tile form over the full range: parameters, both moments, enc_colsq, dec_inv_norm to their bounds; W_enc = W_encT transposed,
    W_enc16T = W_encT.half() and the ``zero`` rows bit for bit"""
    c = AC.make(d_in, clip, step)
    got, before = applied(engine(c), c)
    ratios, msgs = AC.check(c, AC.reference(c), got)
    assert ratios["conservative_inf"] == 0
    for j in np.flatnonzero(c.cls == AC.ZERO):                                 # (check holds W_encT / W_dec; the rest of a zero row as well)
        for q in ("m_W_encT", "v_W_encT", "m_W_dec", "v_W_dec", "W_enc16T"):
            assert same_bits(got[q][j], before[q][j]), (q, j)
        assert same_bits(got["W_enc"][:, j], before["W_enc"][:, j]) and same_bits(got["b_enc"][j], before["b_enc"][j]), j
    verdict(f"apply {c.name}", ratios, msgs)


@pytest.mark.parametrize("d_in", [100, 772])
@pytest.mark.parametrize("lo,mid", [(0, 40), (0, 41)])
def test_apply_on_a_sub_range_leaves_the_rest_alone(d_in, lo, mid):
    """[0, mid) then [mid, 72) at the same adam_step against one full apply: everything outside the range applied keeps its bits (parameters,
    moments, the three encoder copies, enc_colsq, dec_inv_norm; b_dec moves on every call, by contract), and the feature rows of the two
    halves are the full apply's, bit for bit.  include/pv_native.h sets no alignment rule for apply: 41 is on no grid."""
    full_c = AC.make(d_in, "active", 2)
    full, _ = applied(engine(full_c), full_c)
    eng = engine(full_c)
    for j_lo, j_hi in ((lo, mid), (mid, 72)):
        c = AC.make(d_in, "active", 2, j_lo=j_lo, j_hi=j_hi)
        if j_lo:
            # the second half starts from what the first left: its own rows are untouched (held below), the others and b_dec have moved
            for D_, pre in ((c.P, ""), (c.M, "m_"), (c.V, "v_")):
                for key in c.P:
                    D_[key] = got[pre + key].copy()
            eng.adam_step = c.step - 1
        got, before = applied(eng, c)
        ratios, msgs = AC.check(c, AC.reference(c), got)
        outside = np.ones(72, bool)
        outside[j_lo:j_hi] = False
        for q in ("W_encT", "W_dec", "b_enc", "m_W_encT", "m_W_dec", "m_b_enc", "v_W_encT", "v_W_dec", "v_b_enc", "W_enc16T", "enc_colsq", "dec_inv_norm"):
            assert same_bits(got[q][outside], before[q][outside]), (q, j_lo, j_hi)
        assert same_bits(got["W_enc"][:, outside], before["W_enc"][:, outside])
        assert not same_bits(got["b_dec"], before["b_dec"])
        verdict(f"apply {c.name} rows [{j_lo}, {j_hi})", ratios, msgs)
    for q in ("W_encT", "W_enc", "W_dec", "b_enc", "m_W_encT", "m_W_dec", "m_b_enc", "v_W_encT", "v_W_dec", "v_b_enc", "W_enc16T", "enc_colsq",
              "dec_inv_norm"):
        assert same_bits(got[q], full[q]), f"{q}: the two halves differ from the full apply"


@pytest.mark.parametrize("d_in", [100, 260, 1280])
def test_enc_colsq_with_big_rows(d_in, tuning):
    """+inf is mandatory for a row holding an element beyond 6.0e4 or a non-finite one.  The tile form may also report it for the up to three
    rows that share the big row's thread (same 32-feature tile, same row mod 8), the row form may not; every other row is held to its bound."""
    c = AC.make(d_in, "inactive", 2, big=True)
    ref = AC.reference(c)
    for lazy in (False, True):
        tuning("sae_fold", 1)
        got, _ = applied(engine(c, lazy=lazy), c, w_enc=not lazy)
        ratios, msgs = AC.check(c, ref, got, form="rows" if lazy else "tile")
        print(f"[sae-apply] big rows d_in={d_in} {'row' if lazy else 'tile'} form: {int(ratios['conservative_inf'])} finite rows came out +inf "
              f"({len(c.big)} rows hold a big element)")
        if lazy:
            assert ratios["conservative_inf"] == 0
        verdict(f"apply {c.name} {'row' if lazy else 'tile'} form", ratios, msgs)
    sub = AC.make(d_in, "inactive", 2, big=True, j_lo=8, j_hi=72)               # the tiles counted from j_lo = 8
    got, _ = applied(engine(sub), sub)
    ratios, msgs = AC.check(sub, AC.reference(sub), got)
    verdict(f"apply {sub.name} rows [8, 72)", ratios, msgs)


# ------------------------------------------------------------------------------------------------ pending decoder renorm
@pytest.mark.parametrize("d_in", AC.WIDTHS)
def test_renorm_decoder_alone(d_in):
    """rows at norms 2^-10 .. 2^10 through renorm_rows_kernel (DPL_DISPATCH at every width)"""
    c = AC.make(d_in, "inactive", 1, pending=True)
    eng = engine(c, planted=False)
    eng.renorm_decoder()
    torch.cuda.synchronize()
    want, bound = AC.renorm_ref(c.P["W_dec"])
    r = AC._ratios(eng.params["W_dec"].cpu().numpy(), want, bound)
    print(f"[sae-apply] renorm_decoder d_in={d_in}: W_dec={r.max():.3g}")
    j, i = np.unravel_index(int(np.argmax(r)), r.shape)
    assert r.max() <= 1.0, f"feature row {j} (norm 2^{np.log2(np.linalg.norm(c.P['W_dec'][j].astype(F64))):.0f}) column {i}: ratio {r.max():.3g}"


@pytest.mark.parametrize("d_in,lo,hi", [(100, 0, 72), (260, 0, 72), (1280, 0, 72), (772, 0, 40)])
def test_apply_with_a_pending_decoder_renorm(d_in, lo, hi):
    """step(x, renorm_decoder=True) leaves 1 / ||row|| in dec_inv_norm and the rows as they were; the apply behind it must update the RENORMED
    rows (the reference's rn w with the kernel's own rn) and leave dec_inv_norm of the rows it wrote."""
    c = AC.make(d_in, "active", 1000, pending=True, j_lo=lo, j_hi=hi)
    eng = engine(c, planted=False)
    x = torch.from_numpy(np.random.RandomState(d_in).standard_normal((16, d_in)).astype(F32)).cuda()
    eng.step(x, renorm_decoder=True)
    torch.cuda.synchronize()
    assert same_bits(eng.params["W_dec"].cpu().numpy(), c.P["W_dec"]), "the step defers the rewrite of W_dec to apply"
    inv = eng.dec_inv_norm.cpu().numpy()
    want, bound = AC.inv_norm_ref(c.P["W_dec"])
    r0 = AC._ratios(inv, want, bound)
    assert r0.max() <= 1.0, f"dec_inv_norm as the step left it: feature row {int(np.argmax(r0))}, ratio {r0.max():.3g}"
    c.inv_norm = inv
    plant(eng, c)                                                               # (over the step's own gradient and clip norm)
    got, before = applied(eng, c)
    ratios, msgs = AC.check(c, AC.reference(c), got)
    ratios["dec_inv_norm_of_the_step"] = float(r0.max())
    outside = np.ones(72, bool)
    outside[lo:hi] = False
    assert same_bits(got["W_dec"][outside], before["W_dec"][outside]) and same_bits(got["dec_inv_norm"][outside], inv[outside])
    verdict(f"apply {c.name} rows [{lo}, {hi})", ratios, msgs)


# ------------------------------------------------------------------------------------------------ the lazy (row) form
@pytest.mark.parametrize("d_in", [64, 100, 260, 1028, 1280])
@pytest.mark.parametrize("clip", ["disabled", "active"])
def test_lazy_form_against_the_tile_form(d_in, clip, tuning):
    """adam_wenct_kernel (W_enc == NULL) with the bias vectors in its launch (sae_fold 1) and in their own (0), against the tile form on the
    same state.  Clipping disabled (the coefficient is exactly 1): every bit of W_encT, both moments, W_enc16T, b_enc, b_dec is equal; active:
    each is held to the bounds and whether the bits agree is printed.  W_enc is untouched until materialize_w_enc()."""
    c = AC.make(d_in, clip, 2)
    ref = AC.reference(c)
    tile, _ = applied(engine(c), c)
    for fold in (1, 0):
        tuning("sae_fold", fold)
        eng = engine(c, lazy=True)
        got, before = applied(eng, c, w_enc=False)
        ratios, msgs = AC.check(c, ref, got, form="rows")
        assert same_bits(got["W_enc_stale"], before["W_enc"]), "the row form wrote the parameter's own layout"
        eng.materialize_w_enc()
        torch.cuda.synchronize()
        assert same_bits(eng.params["W_enc"].cpu().numpy().T, got["W_encT"]), "materialize_w_enc: W_enc is not W_encT transposed"
        names = ("W_encT", "m_W_encT", "v_W_encT", "W_enc16T", "b_enc", "b_dec", "m_b_enc", "v_b_enc", "m_b_dec", "v_b_dec", "W_dec", "m_W_dec", "v_W_dec")
        differ = [q for q in names if not same_bits(got[q], tile[q])]
        print(f"[sae-apply] lazy d_in={d_in} clip={clip} fold={fold}: bits against the tile form {'equal' if not differ else 'DIFFER in ' + ', '.join(differ)}; "
              f"enc_colsq bits {'equal' if same_bits(got['enc_colsq'], tile['enc_colsq']) else 'differ (another summation order)'}")
        if clip == "disabled":
            assert not differ, differ
        verdict(f"apply {c.name} row form fold={fold}", ratios, msgs)


# ------------------------------------------------------------------------------------------------ sync_shadows
@pytest.mark.parametrize("d_in", [100, 260, 1280])
def test_sync_shadows_both_directions_and_a_sub_range(d_in):
    """the weight classes (fp16 ties, subnormals, 2^-25, 60000) and the big rows through wenc_rows_kernel<1> and <2>: the copies bit for bit,
    enc_colsq to its bound and the ``big`` rule, the rows outside [8, 50) untouched"""
    old, new = AC.make(d_in, "inactive", 1), AC.make(d_in, "inactive", 1, big=True, seed=1)
    for from_transposed in (False, True):
        for lo, hi in ((0, 72), (8, 50)):
            eng = engine(old, planted=False)
            before = snapshot(eng, old)
            expect = old.P["W_encT"].copy()
            expect[lo:hi] = new.P["W_encT"][lo:hi]
            if from_transposed:
                eng.W_encT.copy_(dev(new.P["W_encT"]))                          # (rows outside the range: overwritten here, not by the kernel)
                expect = new.P["W_encT"]
            else:
                eng.params["W_enc"].copy_(dev(new.P["W_encT"].T))
            eng.sync_shadows(from_transposed=from_transposed, j_lo=lo, j_hi=hi)
            got = snapshot(eng, old)
            c = AC.shadow_case(expect, lo, hi)
            got = {q: got[q] for q in ("W_encT", "W_enc16T", "enc_colsq")}
            got.update(W_enc16T_before=before["W_enc16T"], enc_colsq_before=before["enc_colsq"])
            ratios, msgs = AC.check(c, AC.reference(c), got)
            W = eng.params["W_enc"].cpu().numpy()
            if from_transposed:                                                 # W_enc: the columns of the range rewritten, the others as they were
                want = before["W_enc"].copy()
                want[:, lo:hi] = new.P["W_encT"][lo:hi].T
            else:
                want = new.P["W_encT"].T
            fin = np.isfinite(want)
            assert same_bits(W[fin], want[fin]) and not np.isfinite(W[~fin]).any(), "W_enc"
            verdict(f"sync_shadows d_in={d_in} from_transposed={int(from_transposed)} rows [{lo}, {hi})", ratios, msgs)


# ------------------------------------------------------------------------------------------------ sparse-gradient step, then apply
def test_sparse_gradient_step_then_apply_with_live_moments():
    """On the ``boundaries`` pattern with non-zero moments planted on every row: a sparse_grads step into a NaN-poisoned flat_g, the clip norm
    from the step's per-feature terms, apply.  Held to the float64 optimizer step on the float64 gradient of _sae_backward_cases.reference (an
    empty feature's gradient row is 0), the gradient's own bound carried through; the empty rows must have decayed and moved, and be finite."""
    b = SC.planted("boundaries")
    bref = SC.reference(b.P, b.x, b.idx, b.val, b.norm)
    rs = np.random.RandomState(5)
    P = dict(W_encT=np.ascontiguousarray(b.P["W_enc"].T), W_dec=b.P["W_dec"], b_enc=b.P["b_enc"], b_dec=b.P["b_dec"])
    M = {k_: (1e-3 * rs.standard_normal(v.shape)).astype(F32) for k_, v in P.items()}
    V = {k_: (M[k_].astype(F64) ** 2 * (1.0 + rs.random_sample(M[k_].shape)) * (1 + 4 * AC.U)).astype(F32) for k_ in P}
    G = dict(W_encT=bref["gW_enc"], W_dec=bref["gW_dec"], b_enc=bref["gb_enc"], b_dec=bref["gb_dec"])
    eng = NativeSAE(dev(b.P["W_enc"]), dev(P["W_dec"]), dev(P["b_enc"]), dev(P["b_dec"]), b.k, b.norm, b.n)
    for key in P:
        eng._m[key].copy_(dev(M[key]))
        eng._v[key].copy_(dev(V[key]))
    eng.adam_step = 6
    eng.flat_g.fill_(float("nan"))
    eng.step(dev(b.x), sparse_grads=True)
    eng.grad_sqnorm(from_step=True)
    torch.cuda.synchronize()
    sq = float(eng.scalars[3])
    # the clip norm of the step's own (float32) gradient: the unwritten rows of empty features count as 0
    g_own = torch.nan_to_num(eng.flat_g).double().cpu().numpy()
    own = float((g_own ** 2).sum())
    depth = 2 * b.d_in + 2 + 1 + 1 + 6 + 16 + 2                                 # a feature's 2 d_in + 1 squares in any order, then sqnorm_rowsq_kernel
    sq_bound = float(AC.gamma(depth)) * own * AC.SECOND_ORDER
    print(f"[sae-apply] sparse step: scalars[3] from the step's terms, error / bound = {abs(sq - own) / sq_bound:.3g}")
    assert abs(sq - own) <= sq_bound, (sq, own, sq_bound)
    c = AC.Case("sparse_step", P, G, M, V, F32(sq), 7, F32(1e-3), F32(2.0 ** -12), 0, None, cls=np.full(b.d_sae, AC.MIXED))
    c.G_err = dict(W_encT=bref["gW_enc_bound"], W_dec=bref["gW_dec_bound"], b_enc=bref["gb_enc_bound"], b_dec=bref["gb_dec_bound"])
    ref = AC.reference(c)
    assert ref["coef"] < 1.0
    before = snapshot(eng, c)
    eng.apply(1e-3, 2.0 ** -12)
    got = snapshot(eng, c)
    for q in ("W_enc16T", "enc_colsq", "dec_inv_norm"):
        got[q + "_before"] = before[q]
    ratios, msgs = AC.check(c, ref, got)
    empty = bref["counts"] == 0
    assert int(empty.sum()) > 100
    for key in ("W_encT", "W_dec", "b_enc"):
        assert np.isfinite(got[key][empty]).all() and np.isfinite(got["m_" + key][empty]).all() and np.isfinite(got["v_" + key][empty]).all(), key
        assert (got["m_" + key][empty] != before["m_" + key][empty]).all() and (got["v_" + key][empty] != before["v_" + key][empty]).all(), key
        moved = got[key][empty] != before[key if key != "W_encT" else "W_encT"][empty]
        assert moved.mean() > 0.99, (key, moved.mean())                         # (lr m / sqrt(v) ~ 1e-3: a move under half an ulp of the weight is rare)
    verdict("sparse_grads step on boundaries, live moments, apply", ratios, msgs)


# ------------------------------------------------------------------------------------------------ clip norms
def _sq_check(label, got, terms, depth):
    want, bound = AC.sqnorm_bound(terms, depth)
    r = abs(float(got) - want) / bound if np.isfinite(got) else float("inf")
    print(f"[sae-apply] {label}: scalars[3] error / bound = {r:.3g}")
    assert r <= 1.0, (label, float(got), want, bound)


def test_grad_sqnorm_with_one_dominant_element_per_region():
    """pv_sae_grad_sqnorm over the flat buffer of a transcoder with W_skip at d_in = 100 (six regions, 24 572 elements: a ragged last
    vector of the last sweep), one element 2^40 times the rest in each region in turn"""
    c = AC.make(100, "inactive", 1, extras="transcoder")
    eng = engine(c)
    assert eng.n_flat == 2 * 7200 + 72 + 100 + 100 + 10000
    base = eng.flat_g.clone()
    for key in ("W_encT", "W_dec", "b_enc", "b_dec", "b_dec_out", "W_skip", None):
        eng.flat_g.copy_(base)
        if key is not None:
            eng._g[key].view(-1)[eng._g[key].numel() - 1] = 2.0 ** 40 * 1e-3
        eng.scalars[3] = float("nan")
        eng.grad_sqnorm()
        torch.cuda.synchronize()
        _sq_check(f"grad_sqnorm, dominant element in {key}", eng.scalars[3].item(), eng.flat_g.double().cpu().numpy(), AC.sqnorm_depth(eng.n_flat))


@pytest.mark.parametrize("d_in", [100, 1280])
def test_grad_sqnorm_rows(d_in):
    c = AC.make(d_in, "inactive", 1)
    eng = engine(c)
    for lo, hi in ((0, 40), (40, 72), (4, 6)):
        for with_b_dec in (False, True):
            eng.sq_partial.fill_(float("nan"))
            eng.scalars[3] = float("nan")
            eng.grad_sqnorm_rows(lo, hi, with_b_dec)
            torch.cuda.synchronize()
            terms = np.concatenate([c.G["W_encT"][lo:hi].ravel(), c.G["W_dec"][lo:hi].ravel(), c.G["b_enc"][lo:hi]] + ([c.G["b_dec"]] if with_b_dec else []))
            _sq_check(f"grad_sqnorm_rows d_in={d_in} [{lo}, {hi}) b_dec={int(with_b_dec)}", eng.scalars[3].item(), terms,
                      AC.sqnorm_depth((hi - lo) * d_in, grid=384))


def test_grad_sqnorm_from_a_planted_backward_step():
    b = SC.planted("grid_odd")
    eng = NativeSAE(dev(b.P["W_enc"]), dev(b.P["W_dec"]), dev(b.P["b_enc"]), dev(b.P["b_dec"]), b.k, b.norm, b.n)
    eng.step(dev(b.x))
    eng.grad_sqnorm(from_step=True)
    torch.cuda.synchronize()
    _sq_check("grad_sqnorm(from_step=True) behind grid_odd", eng.scalars[3].item(), eng.flat_g.double().cpu().numpy(), 2 * b.d_in + 2 + 1 + 1 + 6 + 16 + 2)
    from_step = eng.scalars[3].item()
    eng.grad_sqnorm()                                                          # the full pass over the same buffer
    torch.cuda.synchronize()
    _sq_check("grad_sqnorm() behind grid_odd", eng.scalars[3].item(), eng.flat_g.double().cpu().numpy(), AC.sqnorm_depth(eng.n_flat))
    assert from_step > 0


# ------------------------------------------------------------------------------------------------ transcoder and gated engines
def test_transcoder_with_w_skip_at_100():
    """b_dec_out and the 10 000 elements of W_skip (39 whole 256-element blocks + 16) through adam_vec_kernel"""
    c = AC.make(100, "active", 1000, extras="transcoder")
    got, _ = applied(engine(c), c)
    ratios, msgs = AC.check(c, AC.reference(c), got)
    assert {"W_skip", "m_W_skip", "v_W_skip", "b_dec_out"} <= set(ratios)
    verdict(f"apply {c.name}", ratios, msgs)


def test_gated_engine_and_its_refused_sub_range():
    """the three gated vectors to the same bounds; apply(j_lo=0, j_hi=40) on a gated engine must return the error and leave every parameter,
    moment, shadow and adam_step as they were"""
    c = AC.make(260, "active", 2, extras="gated")
    eng = engine(c)
    before = snapshot(eng, c)
    with pytest.raises(N.NativeError, match="whole feature range"):
        eng.apply(float(c.lr), float(c.max_grad_norm), 0, 40)
    after = snapshot(eng, c)
    assert eng.adam_step == c.step - 1, "a refused apply is no step"
    changed = [q for q in before if not same_bits(before[q], after[q])]
    assert not changed, f"the refused call wrote {changed}"
    got, _ = applied(eng, c)
    ratios, msgs = AC.check(c, AC.reference(c), got)
    assert {"b_gate", "r_mag", "b_mag", "v_r_mag"} <= set(ratios)
    verdict(f"apply {c.name}", ratios, msgs)
