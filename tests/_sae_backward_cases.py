"""Planted firing patterns for the k-sparse SAE backward (the CSR by feature, the 16-pair chunks of the short lists, the long lists in
their two segment forms), a float64 reference computed from the (idx, val) pairs, per-element bounds, a checker, and a float32 twin of
the kernels' structure with the slips it can be told to make.  numpy / scipy on the CPU, importable without a GPU.

The GPU suite otherwise feeds the backward ``synth_sae_batch`` and compares whole tensors with ``rel_fro < 1e-4``: at the shapes it uses no
list is ever cut by pair count (that form starts at 37 377 tokens), no hole reaches a backward, the 64 / 65-pair boundary is met by
accident, and one wrong row hides under the largest row's norm (tests/test_sae_backward_cases_cpu.py shows which slips that lets through).

Two ways to plant a pattern
---------------------------
``planted(name)``  for ``pv_sae_step`` / ``relu_step`` (normalisation "none"): d_in = 64 = C class dimensions (32; 48 in ``count_cut``) + free dimensions.  Token n is in
    class c(n): x[n, c(n)] = s_n on a 1/16 grid in [1, 2), the other class dimensions 0, the free dimensions 3 randn.  W_enc[c] is the class's
    score row -- its selected features 1 + slot / 8, every other feature a distinct negative: the k largest -(r + 1) / 4, the rest in (-4, -3] --, the free rows of W_enc are 0,
    b_enc = 0, b_dec = 0 on the class dimensions.  So hidden_pre[n] = s_n W_enc[c(n)] EXACTLY in any precision and summation order (one
    non-zero product of two short binary fractions), the top-k set of every token is known, the gap between the k-th and the (k+1)-th
    pre-activation is >= 1/4, and a class with fewer than k selected features leaves holes (kept slots with value 0).
``injected(name, d_in)``  for ``encode_topk -> tp_partial -> tp_finish`` on a one-rank shard (LayerNorm on, ``synth_sae_batch`` tokens): the
    (idx, val) pairs themselves -- idx distinct within a token, kept values on a 1/64 grid in (0, 4], holes exact 0 and a few negatives (a pair
    with value <= 0 is a hole by include/pv_native.h and must contribute nothing anywhere).

The patterns (``PATTERNS``; k = 8, d_sae = 512 unless said otherwise; L = a feature's list length)
``boundaries``   n 300: L in {0, 1, 15, 16, 17, 26, 33, 63, 64, 65, 96, 97, 300} -- one feature on every token, 63 + 33 and 64 + 33 by two
                 classes sharing a feature, 3 holes.  ``boundaries_2048``: the same at d_sae 2048 (the filtered encoder; planted only)
``grid16`` / ``grid_odd``  feature 0 empty; the first list (feature 1) long with 80 pairs, so feature 2's list of exactly 16 sits on the
                 16-pair grid [80, 96) and feature 3's starts on a multiple of 16; the last non-empty list (feature d_sae - 1) long; the
                 total a multiple of 16 (1328) or not (1368)
``all_long65`` / ``all_long64``  n 65 / 64, every token keeps the same 8 features: all lists long and on every token (all eight token
                 ranges full), or all exactly BWD_LMAX (no long list, no segment)
``no_pairs``     n 96, every value <= 0: total 0, every chunk cut beyond the total, d_sae empty rows
``one_range300`` / ``one_range65`` / ``one_range560``  a 70-pair list on the first and one on the last min(70, n) tokens, one (``bnd``) holding
                 the tokens r rs - 1 and r rs of every range boundary r = 1..7 (rs = ceil(n / 8)) filled up to 65 pairs where n allows, the
                 rest short; n no multiple of 8 at 300 and 65; at 560 rs = 70 and the two 70-pair lists lie in ONE range each (seven empty
                 segments)
``count_cut``    n 37 377, the smallest n beyond the token-range form: L = 64, 65 (segments 32, 32, 1), 96, 97, 129, n; 40 small classes
                 whose 280 short lists hold a few thousand pairs; most slots holes

The reference and the bounds (``reference``): float64 of oracle/sae_oracle.py's forward and backward, computed from the pairs with the gate
val > 0.  With u = 2^-24 and gamma(m) = m u / (1 - m u) (any summation order of m operations), every kernel quantity carries a bound
assembled operation by operation from the absolute sums the float64 computation provides (first order in u; ``SECOND_ORDER`` covers the
rest):
  LayerNorm statistics  mu: gamma(d) mean|x|;  x - mu: mu_err + u |x - mu|;  the centred sum of squares: gamma(d + 1) q + 2 sum |xc| xc_err;
                        std = sqrt(q / (d - 1)): v_err / std + 2 u std (the derivative 1 / (2 std), doubled);  sae_in follows by the quotient rule
  loss normaliser       the same through the batch mean (gamma(n + 2) mean_n |x|)
  decode                acc = sum_s a_s W_dec[j_s]: gamma(k + 2) (sum |a W| + |b_dec|);  LN-out, the residual e, dY = gs e / nf sd: the
                        product and quotient rules + 6 u |dY|;  dh = dY . W_dec[j]: gamma(d + 1) sum |dY W| + sum dY_err |W|
  gW_dec[j, e]          gamma(m) sum_p |a_p| |dY[n_p, e]| + sum_p (|a_p| dY_err[n_p, e] + a_err_p |dY[n_p, e]|),  m = L + the segment combines
  gW_enc^T[j, e]        the same with dh and sae_in;  gb_enc[j] with dh alone;  gb_dec with gamma(n + d_sae + 4) over both of its sums
  loss, sae_out         from the residual's error;  partial (the feature-parallel step's reconstruction without b_dec): gamma(k + 1) sum |a W|
a_err is 0 in every case here: planted values are exact by construction, injected ones are the caller's.  No constant is measured.

``check`` returns the worst error / bound per quantity -- inf for NaN where a number belongs or a number where poison belongs -- and the
messages naming feature, list length and worst element; ``passes``: every ratio <= 1.

``twin``: a float32 numpy port of the kernels' structure (offsets, chunk cuts snapped to list ends, long-list registration, the token-range
and the count-cut segment forms, the segment combine, fp32 accumulation in list order); ``SLIPS`` are the wrong versions of it.
"""
import concurrent.futures
import functools
import math

import numpy as np
import scipy.sparse as sp

from oracle import sae_oracle as O
from vit_prisma_amd.synth import synth_sae_batch, synth_sae_state

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
SECOND_ORDER = 1.0 + 2.0 ** -10
LN_EPS = 1e-5
BWD_CH, BWD_LMAX, BWD_SEG, BWD_RANGES, SEG_WAVES = 16, 64, 32, 8, 8
RANGED_MAX_TOKENS = 37376
K = 8
WIDTHS = (64, 100, 264, 1156)                      # injected pairs: V4 = 1, 1 ragged, a second vector of 8 columns, 5 ragged
PATTERNS = ("boundaries", "grid16", "grid_odd", "all_long65", "all_long64", "no_pairs", "one_range300", "one_range65", "one_range560",
            "count_cut")
BOUNDARY_LENGTHS = (0, 1, 15, 16, 17, 26, 33, 63, 64, 65, 96, 97, 300)
QUANTITIES = ("sae_out", "partial", "loss", "gW_dec", "gW_enc", "gb_enc", "gb_dec")


def gamma(m):
    m = np.asarray(m, F64)
    return m * U / (1.0 - m * U)


def long_ranged(n):
    """sae_long_ranged of csrc/sae_bwd.hip: the token-range form sorts a list through an n x 4-byte LDS array"""
    return n * 4 + 4096 <= 150 * 1024


assert long_ranged(RANGED_MAX_TOKENS) and not long_ranged(RANGED_MAX_TOKENS + 1)


def combines(L, n, ranged=None):
    """operations beyond the L of the list itself that a long list's row goes through: the eight waves of a token-range segment and the
    eight segments, or the ceil(L / 32) count-cut segments"""
    L = np.asarray(L)
    ranged = long_ranged(n) if ranged is None else ranged
    extra = (SEG_WAVES + BWD_RANGES) if ranged else (L + BWD_SEG - 1) // BWD_SEG
    return np.where(L > BWD_LMAX, extra, 0)


def _rng(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + (sum(map(ord, k)) if isinstance(k, str) else int(k))) % (2 ** 31)
    return np.random.RandomState(seed)


class Case:
    """P: float32 parameters; x [n, d_in] float32; idx [n, k] int32 / val [n, k] float32: the pairs (planted: what the kernel must select, in
    value-descending order; injected: what the caller hands over); norm; lengths [d_sae]: the list lengths the case claims; named: the
    features of the lists the pattern is about."""

    def __init__(self, name, kind, P, x, idx, val, norm, lengths, named, holes):
        self.name, self.kind, self.P, self.x, self.idx, self.val, self.norm = name, kind, P, x, idx, val, norm
        self.lengths, self.named, self.holes = lengths, named, holes
        self.n, self.d_in = x.shape
        self.k = idx.shape[1]
        self.d_sae = P["W_dec"].shape[0]

    def __repr__(self):
        return f"<{self.kind} {self.name} n={self.n} d_in={self.d_in} d_sae={self.d_sae}>"


# ------------------------------------------------------------------------------------------------------------ pattern descriptions
def range_size(n):
    return (n + BWD_RANGES - 1) // BWD_RANGES


def boundary_tokens(n):
    rs = range_size(n)
    return sorted({t for r in range(1, BWD_RANGES) for t in (r * rs - 1, r * rs) if 0 <= t < n})


def _spread(tokens, pieces):
    """cut a token list into `pieces` interleaved parts (every part reaches over the whole list)"""
    return [tokens[i::pieces] for i in range(pieces)]


def pattern_classes(name, d_sae=512):
    """-> (n, classes): classes = [(tokens, positive features in slot order)], a partition of the n tokens; every class has at most K
    positive features.  Planted cases use it as it is; injected cases turn it into pairs."""
    last = d_sae - 1
    nxt = [100]

    def own(m):
        nxt[0] += m
        return list(range(nxt[0] - m, nxt[0]))

    if name in ("boundaries", "boundaries_2048"):
        sizes = (65, 64, 63, 33, 17, 16, 15, 1, 26)
        order = _rng("boundaries").permutation(300)
        toks, o = [], 0
        for s in sizes:
            toks.append(sorted(order[o:o + s].tolist()))
            o += s
        sh97, sh96 = 7, 9
        feats = [[5] + own(7), [5] + own(6) + [sh97], [5] + own(6) + [sh96], [5, sh97, sh96] + own(5), [5] + own(7), [5] + own(7),
                 [5] + own(7), [5] + own(4), [5] + own(7)]
        return 300, list(zip(toks, feats))
    if name in ("grid16", "grid_odd"):
        sizes = [80, 16, 70] + ([5] if name == "grid_odd" else [])
        feats = [[1] + list(range(10, 17)), [2, 3] + list(range(20, 26)), list(range(last - 7, last + 1)), list(range(30, 38))]
        n = sum(sizes)
        order = _rng(name).permutation(n)
        toks, o = [], 0
        for s in sizes:
            toks.append(sorted(order[o:o + s].tolist()))
            o += s
        return n, list(zip(toks, feats))
    if name in ("all_long65", "all_long64"):
        n = int(name[-2:])
        return n, [(list(range(n)), [3, 64, 65, 127, 128, 300, 510, 511])]
    if name == "no_pairs":
        return 96, [(list(range(0, 96, 3)), []), (list(range(1, 96, 3)), []), (list(range(2, 96, 3)), [])]
    if name.startswith("one_range"):
        n = int(name[len("one_range"):])
        m = min(70, n)
        first, lastt, bnd = set(range(m)), set(range(n - m, n)), set(boundary_tokens(n))
        rest = [t for t in range(n) if t not in first and t not in lastt and t not in bnd]
        fill = set(rest[::max(1, len(rest) // 51)][:max(0, 65 - len(bnd))]) if rest else set()      # the bnd list made long where n allows
        F_FIRST, F_LAST, F_BND = 40, 41, 42
        atoms = {}
        for t in range(n):
            key = (t in first, t in lastt, t in bnd or t in fill)
            atoms.setdefault(key, []).append(t)
        classes = []
        for key, toks in sorted(atoms.items()):
            base = [f for f, on in zip((F_FIRST, F_LAST, F_BND), key) if on]
            for part in _spread(toks, (len(toks) + 39) // 40):                 # own features stay short: at most 40 tokens a class
                classes.append((part, base + own(K - len(base) - (1 if len(classes) % 3 == 2 else 0))))
        return n, classes
    if name == "count_cut":
        n = RANGED_MAX_TOKENS + 1
        order = _rng("count_cut").permutation(n)
        classes, o = [], 0
        F_ALL = 6
        for L, f in ((64, 20), (65, 21), (129, 24)):
            classes.append((sorted(order[o:o + L].tolist()), [F_ALL, f]))
            o += L
        # 96 = 63 + 33 and 97 = 64 + 33 as in `boundaries`
        for L, fs in ((63, [22]), (64, [23]), (33, [22, 23])):
            classes.append((sorted(order[o:o + L].tolist()), [F_ALL] + fs + own(1)))
            o += L
        for i in range(40):
            L = 1 + (i * 37) % 63
            classes.append((sorted(order[o:o + L].tolist()), [F_ALL] + own(7)))
            o += L
        classes.append((sorted(order[o:].tolist()), [F_ALL]))                  # the bulk: one kept feature, seven holes
        return n, classes
    raise KeyError(name)


def named_lists(name, d_sae=512):
    """the features the pattern is about -> the list length it claims for them"""
    if name in ("boundaries", "boundaries_2048"):
        return {5: 300, 7: 97, 9: 96}
    if name in ("grid16", "grid_odd"):
        return {0: 0, 1: 80, 2: 16, 3: 16, d_sae - 1: 70}
    if name in ("all_long65", "all_long64"):
        n = int(name[-2:])
        return {j: n for j in (3, 64, 65, 127, 128, 300, 510, 511)}
    if name == "no_pairs":
        return {}
    if name.startswith("one_range"):
        n = int(name[len("one_range"):])
        return {40: min(70, n), 41: min(70, n), 42: {300: 65, 65: 14, 560: 65}[n]}
    if name == "count_cut":
        return {6: RANGED_MAX_TOKENS + 1, 20: 64, 21: 65, 22: 96, 23: 97, 24: 129}
    raise KeyError(name)


def class_lengths(classes, d_sae):
    L = np.zeros(d_sae, np.int64)
    for toks, feats in classes:
        for f in feats:
            L[f] += len(toks)
    return L


# ------------------------------------------------------------------------------------------------------------ planted classes
def planted(name, d_in=64, seed=0):
    d_sae = 2048 if name.endswith("_2048") else 512
    n, classes = pattern_classes(name, d_sae)
    C = 32 if len(classes) <= 32 else 48                                      # class dimensions (count_cut has 47 classes); the rest are free
    assert len(classes) <= C <= d_in - 8, (name, C)
    rs = _rng("planted", name, seed)
    W_enc = np.zeros((d_in, d_sae), F32)
    idx = np.zeros((n, K), np.int32)
    val = np.zeros((n, K), F32)
    x = np.zeros((n, d_in), F32)
    x[:, C:] = (3.0 * rs.standard_normal((n, d_in - C))).astype(F32)
    s = (1.0 + rs.randint(0, 16, size=n) / 16.0).astype(F32)
    holes = 0
    for c, (toks, feats) in enumerate(classes):
        assert len(feats) <= K and len(set(feats)) == len(feats)
        others = np.setdiff1d(np.arange(d_sae), feats)
        others = others[rs.permutation(others.size)]
        # distinct negatives: the K largest 1/4 apart (what a class with fewer than K selected features keeps as holes), the others
        # in (-4, -3].  Small and far from 0 on purpose: the error band of the ReLU step's fp16 filter grows with the largest column
        # norm of W_enc, and every feature inside the band around 0 is a candidate it has to hold (32 slots per token and 256 features,
        # 4096 per 256 x 256 tile, or the step runs on the dense GEMMs instead)
        W_enc[c, others[:K]] = -(np.arange(K) + 1.0) / 4.0
        W_enc[c, others[K:]] = -(3.0 + np.arange(others.size - K) / float(d_sae))
        for slot, f in enumerate(feats):
            W_enc[c, f] = 1.0 + slot / 8.0
        sel = list(reversed(feats)) + others[:K - len(feats)].tolist()         # value descending: the kept slots, then the holes
        toks = np.asarray(toks, np.int64)
        x[toks, c] = s[toks]
        idx[toks] = np.asarray(sel, np.int32)
        val[toks] = np.maximum(s[toks, None] * W_enc[c, sel][None, :], 0.0)
        holes += toks.size * (K - len(feats))
    st = synth_sae_state(d_in, d_sae, 3)
    b_dec = st["b_dec"].copy()
    b_dec[:C] = 0.0
    P = dict(W_enc=W_enc, W_dec=st["W_dec"].copy(), b_enc=np.zeros(d_sae, F32), b_dec=b_dec)
    return Case(name, "planted", P, x, idx, val, "none", class_lengths(classes, d_sae), named_lists(name, d_sae), holes)


# ------------------------------------------------------------------------------------------------------------ injected pairs
@functools.lru_cache(maxsize=None)
def _injected_pairs(name, seed, negatives):
    d_sae = 512
    n, classes = pattern_classes(name, d_sae)
    rs = _rng("injected", name, seed)
    idx = np.zeros((n, K), np.int32)
    val = np.zeros((n, K), F32)
    holes = 0
    for toks, feats in classes:
        toks = np.asarray(toks, np.int64)
        m, nh = toks.size, K - len(feats)
        key = rs.random_sample((m, d_sae))
        key[:, feats] = 2.0
        fill = np.argsort(key, axis=1)[:, :nh]                                 # hole slots: any other features, distinct within the token
        row = np.concatenate([np.broadcast_to(np.asarray(feats, np.int64), (m, len(feats))), fill], axis=1)
        v = np.concatenate([rs.randint(1, 257, size=(m, len(feats))) / 64.0, np.zeros((m, nh))], axis=1)
        p = np.argsort(rs.random_sample((m, K)), axis=1)                        # kept pairs and holes in any slot
        idx[toks], val[toks] = np.take_along_axis(row, p, axis=1), np.take_along_axis(v, p, axis=1)
        holes += m * nh
    hole_pos = np.argwhere(val == 0)
    if len(hole_pos):
        for i, h in enumerate(rs.choice(len(hole_pos), min(negatives, len(hole_pos)), replace=False)):
            val[tuple(hole_pos[h])] = -(1.0 + (i % 7)) / 4.0                   # a negative value is a hole too
    idx.setflags(write=False)
    val.setflags(write=False)
    return n, idx, val, class_lengths(classes, d_sae), holes


def injected(name, d_in=64, seed=0, negatives=5):
    """the same pairs at every width"""
    d_sae = 512
    n, idx, val, lengths, holes = _injected_pairs(name, seed, negatives)
    P = {k_: v.copy() for k_, v in synth_sae_state(d_in, d_sae, 1).items()}
    O.renorm_decoder(P)
    x = synth_sae_batch(n, d_in, seed=7)
    return Case(name, "injected", P, x, idx, val, "layer_norm", lengths, named_lists(name, d_sae), holes)


# ------------------------------------------------------------------------------------------------------------ float64 reference
def _pair_dots(dY, dY_err, Wd, tok, jj, chunk=16384):
    """per kept pair: dY[n] . W_dec[j], sum |dY| |W_dec|, sum dY_err |W_dec|"""
    out = np.zeros((3, tok.size))
    for i in range(0, tok.size, chunk):
        t, w = tok[i:i + chunk], Wd[jj[i:i + chunk]]
        out[0, i:i + chunk] = np.einsum("pd,pd->p", dY[t], w)
        np.abs(w, out=w)
        out[1, i:i + chunk] = np.einsum("pd,pd->p", np.abs(dY[t]), w)
        out[2, i:i + chunk] = np.einsum("pd,pd->p", dY_err[t], w)
    return out


def reference(P, x, idx, val, norm, n_global=None, l1=0.0, ranged=None, block=2048):
    """float64 forward and backward from the pairs (gate val > 0), the bound of every quantity beside it (``<name>_bound``).
    gb_dec in the shard form colsum(dY) - W_enc gb_enc (one rank: the whole gradient).  Tokens are walked in blocks (the arithmetic is
    per token; only the sums over the lists and over the batch cross blocks)."""
    P = {k_: np.asarray(v, F64) for k_, v in P.items()}
    x_all = np.asarray(x)
    val_all = np.asarray(val, F64)
    idx_all = np.asarray(idx, np.int64)
    n, d = x_all.shape
    k = idx_all.shape[1]
    d_sae = P["W_dec"].shape[0]
    ng = n if n_global is None else n_global
    mode = O.norm_mode(norm)
    assert mode in ("none", "layer_norm")
    Wd, Wd_abs, b_dec = P["W_dec"], np.abs(P["W_dec"]), P["b_dec"]
    bm = x_all.mean(axis=0, keepdims=True, dtype=F64)
    bm_err = gamma(n + 2) * np.abs(x_all).mean(axis=0, keepdims=True, dtype=F64)
    gs = 2.0 / (ng * d)
    add = l1 / ng
    full = {q_: np.zeros((n, d)) for q_ in ("sae_out", "sae_out_bound", "dY", "dY_err", "sae_in", "partial", "partial_bound")}
    rows = {q_: np.zeros((n, 1)) for q_ in ("mu", "std", "norm_factor")}
    dh, dh_err = np.zeros((n, k)), np.zeros((n, k))
    acc_names = ("gW_dec", "gW_dec_abs", "gW_dec_in", "gW_enc", "gW_enc_abs", "gW_enc_in")
    S = {q_: np.zeros((d_sae, d)) for q_ in acc_names}
    Sb = np.zeros((3, d_sae))
    col = np.zeros((3, d))
    t_sum = t_err_sum = a_sum = 0.0

    def one_block(b0):
        sl = slice(b0, min(b0 + block, n))
        x = x_all[sl].astype(F64)
        m = x.shape[0]
        if mode == "layer_norm":
            mu = x.mean(axis=1, keepdims=True)
            xc = x - mu
            q = (xc ** 2).sum(axis=1, keepdims=True)
            v = q / (d - 1)
            std = np.sqrt(v)
            sdp = std + LN_EPS
            xh = xc / sdp
            mu_err = gamma(d) * np.abs(x).mean(axis=1, keepdims=True)
            xc_err = mu_err + U * np.abs(xc)
            q_err = gamma(d + 1) * q + (2 * np.abs(xc) * xc_err + xc_err ** 2).sum(axis=1, keepdims=True)
            v_err = q_err / (d - 1) + 2 * U * v
            std_err = v_err / std + 2 * U * std
            sdp_err = std_err + U * sdp
            xh_err = (xc_err + np.abs(xh) * sdp_err) / (sdp - sdp_err) + 2 * U * np.abs(xh)
        else:
            mu, std = np.zeros((m, 1)), np.ones((m, 1))
            mu_err, std_err = np.zeros((m, 1)), np.zeros((m, 1))
            xh, xh_err = x, np.zeros_like(x)
        si = xh - b_dec
        si_err = xh_err + U * np.abs(si)
        # the loss normaliser ||x_n - batch mean||
        c = x - bm
        c_err = bm_err + U * np.abs(c)
        cn = (c ** 2).sum(axis=1, keepdims=True)
        cn_err = gamma(d + 1) * cn + (2 * np.abs(c) * c_err + c_err ** 2).sum(axis=1, keepdims=True)
        nf = np.sqrt(cn)
        nf_err = cn_err / nf + 2 * U * nf
        # decode
        vb, ib = val_all[sl], idx_all[sl]
        live = vb > 0
        a = vb[live]
        tok = np.broadcast_to(np.arange(m)[:, None], ib.shape)[live]          # the kept pairs, token-major: token, feature, activation
        jj = ib[live]
        AT = sp.csr_matrix((a, (tok, jj)), shape=(m, d_sae))
        part_rec, part_abs = AT @ Wd, AT @ Wd_abs
        pre = part_rec + b_dec
        pre_abs = part_abs + np.abs(b_dec)
        pre_err = gamma(k + 2) * pre_abs
        out = pre * std + mu
        out_err = pre_err * std + (np.abs(pre) + pre_err) * std_err + mu_err + 2 * U * (pre_abs * std + np.abs(mu))
        e = out - x
        e_err = out_err + U * np.abs(e)
        rel_nf = nf_err / (nf - nf_err)
        dY = gs * e / nf * std
        dY_err = gs * std / nf * e_err * (1 + rel_nf) + np.abs(dY) * (rel_nf + std_err / std + 6 * U)
        t = e ** 2 / nf
        sums = (t.sum(), ((2 * np.abs(e) * e_err + e_err ** 2) / nf * (1 + rel_nf) + t * rel_nf).sum(), a.sum())
        dot, dot_abs, dot_e = _pair_dots(dY, dY_err, Wd, tok, jj)
        g = dot + add
        g_err = gamma(d + 1) * dot_abs + dot_e + 2 * U * (np.abs(dot) + add)
        dh[sl][live], dh_err[sl][live] = g, g_err
        # the sums over the lists: sparse [d_sae, tokens] matrices of a, dh and dh's error
        mat = lambda vals: sp.csr_matrix((vals, (jj, tok)), shape=(d_sae, m))
        A, G, Gabs, Gerr = mat(a), mat(g), mat(np.abs(g)), mat(g_err)
        dY_abs, si_abs = np.abs(dY), np.abs(si)
        # (gW_enc transposed: [d_sae, d_in], the layout the kernels write)
        part = dict(gW_dec=A @ dY, gW_dec_abs=A @ dY_abs, gW_dec_in=A @ dY_err, gW_enc=G @ si, gW_enc_abs=Gabs @ si_abs,
                    gW_enc_in=Gabs @ si_err + Gerr @ (si_abs + si_err))
        pb = np.stack([np.asarray(M_.sum(axis=1)).ravel() for M_ in (G, Gabs, Gerr)])
        pc = np.stack([dY.sum(axis=0), dY_abs.sum(axis=0), dY_err.sum(axis=0)])
        for q_, v_ in (("sae_out", out), ("sae_out_bound", out_err), ("dY", dY), ("dY_err", dY_err), ("sae_in", si), ("partial", part_rec),
                       ("partial_bound", gamma(k + 1) * part_abs)):
            full[q_][sl] = v_
        for q_, v_ in (("mu", mu), ("std", std), ("norm_factor", nf)):
            rows[q_][sl] = v_
        return part, pb, pc, sums

    starts = list(range(0, n, block))
    if len(starts) > 2:                                                       # (numpy releases the GIL: blocks side by side, summed in block order)
        with concurrent.futures.ThreadPoolExecutor(max_workers=8) as ex:
            parts = list(ex.map(one_block, starts))
    else:
        parts = [one_block(b0) for b0 in starts]
    for part, pb, pc, sums in parts:
        for q_ in acc_names:
            S[q_] += part[q_]
        Sb += pb
        col += pc
        t_sum, t_err_sum, a_sum = t_sum + sums[0], t_err_sum + sums[1], a_sum + sums[2]
    live = val_all > 0
    counts = np.bincount(idx_all[live], minlength=d_sae)
    gm = gamma(counts + combines(counts, n, ranged))
    mse = t_sum / (ng * d)
    l1_loss = l1 * a_sum / ng
    loss = mse + l1_loss
    r = dict(full, **rows)
    r.update(loss=loss, mse_loss=mse, l1_loss=l1_loss, dh=dh, dh_err=dh_err, counts=counts, l0=float(live.sum()) / n, live=live, idx=idx_all)
    r["loss_bound"] = (t_err_sum + gamma(n + d + 8) * t_sum) / (ng * d) + gamma(n * k + 4) * l1_loss + U * loss
    r["gW_dec"], r["gW_dec_bound"] = S["gW_dec"], gm[:, None] * S["gW_dec_abs"] + S["gW_dec_in"]
    r["gW_enc"], r["gW_enc_bound"] = S["gW_enc"], gm[:, None] * S["gW_enc_abs"] + S["gW_enc_in"]
    r["gb_enc"], r["gb_enc_bound"] = Sb[0], gm * Sb[1] + Sb[2]
    We = P["W_enc"]
    r["gb_dec"] = col[0] - We @ r["gb_enc"]
    r["gb_dec_bound"] = gamma(n + d_sae + 4) * (col[1] + np.abs(We) @ np.abs(r["gb_enc"])) + col[2] + np.abs(We) @ r["gb_enc_bound"]
    for q_ in QUANTITIES:
        r[q_ + "_bound"] = r[q_ + "_bound"] * SECOND_ORDER
    return r


# ------------------------------------------------------------------------------------------------------------ the checker
def _ratios(got, ref, bound):
    got = np.asarray(got, F64)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    r = np.where(np.isfinite(got), r, np.inf)
    return r


def check(ref, got, poison=None):
    """got: sae_out [n, d] (optional), loss, l0, gW_dec / gW_enc [d_sae, d], gb_enc, gb_dec, fire_count, idx [n, k] (and val where the kernel
    selected them: ``val``, compared exactly).  poison = "dense": the gradient buffers were NaN before the step -- rows of empty features
    must be exact zeros;  "sparse": PV_SAE_SPARSE_GRADS -- exactly those rows must still be NaN (gb_enc of an empty feature is 0 in both).
    -> (ratios {quantity: worst error / bound, exact checks: 0 or inf}, messages)"""
    ratios, msgs = {}, []
    counts = ref["counts"]
    empty = counts == 0

    def exact(name, ok, what):
        ratios[name] = 0.0 if ok else math.inf
        if not ok:
            msgs.append(f"{name}: {what() if callable(what) else what}")

    if "idx" in got:
        gi, ri = np.asarray(got["idx"], np.int64), ref["idx"]
        if "val" in got:                                                      # the kernel's own selection: sets of all k slots, values exact
            same = np.array_equal(np.sort(gi, axis=1), np.sort(ri, axis=1))
            bad = np.flatnonzero((np.sort(gi, axis=1) != np.sort(ri, axis=1)).any(axis=1)) if gi.shape == ri.shape else [-1]
            exact("index_sets", same, f"token {bad[:1]} keeps another set")
            if same:
                o1, o2 = np.argsort(gi, axis=1), np.argsort(ri, axis=1)
                gv = np.take_along_axis(np.asarray(got["val"], F64), o1, axis=1)
                rv = np.take_along_axis(np.asarray(got["val_ref"], F64), o2, axis=1)
                exact("values", np.array_equal(gv, rv), f"kept values differ at token {np.argwhere(gv != rv)[:1].tolist()}")
    if "fire_count" in got:
        fc = np.asarray(got["fire_count"], F64)
        j = np.flatnonzero(fc != counts)
        exact("fire_count", j.size == 0, f"feature {j[:1]}: {fc[j[:1]]} pairs counted, list length {counts[j[:1]]}")
    if "l0" in got:
        want = F32(F64(counts.sum()) / ref["dY"].shape[0])
        exact("l0", F32(got["l0"]) == want, f"scalars[2] = {got['l0']!r}, float32(pairs / n) = {want!r}")
    for name in ("act_freq_scores", "n_fwd_since_fired"):
        if name in got:
            j = np.flatnonzero(np.asarray(got[name], F64) != np.asarray(got[name + "_ref"], F64))
            exact(name, j.size == 0, f"feature {j[:1]} (list length {counts[j[:1]]})")
    for q_ in ("sae_out", "partial", "gW_dec", "gW_enc", "gb_enc", "gb_dec", "loss"):
        if q_ not in got:
            continue
        g = np.asarray(got[q_], F64)
        per_feature = q_ in ("gW_dec", "gW_enc", "gb_enc")
        r = _ratios(g, ref[q_], ref[q_ + "_bound"])
        if per_feature and poison == "sparse" and q_ != "gb_enc":
            rows = empty
            still = np.isnan(g[rows]).all()
            exact(q_ + "_poison", bool(still), lambda: f"a row of an empty feature was written under sparse_grads "
                  f"(feature {np.flatnonzero(rows)[~np.isnan(g[rows]).all(axis=1)][:1]}, list length 0)")
            r = r[~rows]
            feat_of = np.flatnonzero(~rows)
        else:
            feat_of = np.arange(counts.size)
        if per_feature and poison is not None:
            z = g[empty] if (poison == "dense" or q_ == "gb_enc") else None
            if z is not None:
                exact(q_ + "_empty_rows", bool((z == 0).all()),
                      lambda: f"feature {np.flatnonzero(empty)[(z != 0).reshape(z.shape[0], -1).any(axis=1)][:1]} (list length 0) is not exactly 0")
        worst = float(r.max()) if r.size else 0.0
        ratios[q_] = worst
        if not worst <= 1.0:
            w = np.unravel_index(int(np.argmax(np.where(np.isnan(r), np.inf, r))), r.shape)
            if per_feature:
                j = int(feat_of[w[0]])
                full = (j,) + tuple(int(i) for i in w[1:])
                msgs.append(f"{q_}: feature {j} (list length {int(counts[j])}) element {full}: got {g[full]!r}, float64 {ref[q_][full]!r}, "
                            f"bound {ref[q_ + '_bound'][full]:.3e}, ratio {worst:.3g}")
            else:
                msgs.append(f"{q_}: element {tuple(int(i) for i in w)}: got {g[w] if g.ndim else g!r}, float64 "
                            f"{ref[q_][w] if g.ndim else ref[q_]!r}, ratio {worst:.3g}")
    return ratios, msgs


def passes(ratios):
    return all(v <= 1.0 for v in ratios.values())


def fmt(ratios):
    return " ".join(f"{k_}={v:.3g}" for k_, v in ratios.items())


# ------------------------------------------------------------------------------------------------------------ the float32 twin
SLIPS = ("segment_last_pair_dropped", "list_of_64_owned_by_nobody", "list_of_65_through_the_64_lane_sort", "chunk_cut_inside_a_list",
         "holes_counted_and_filled", "negative_value_live", "range_boundary_token_in_neither_range", "long_combine_stops_at_4_floor",
         "last_vector_dropped_at_ragged_d_in", "seg_b_not_summed_into_gb_enc", "a_from_the_neighbouring_slot", "empty_rows_left_stale",
         "token_is_p_mod_k")


def _seqsum(rows):
    """fp32 sum of the rows in the order given (np.cumsum accumulates sequentially in the array's dtype)"""
    if rows.shape[0] == 0:
        return np.zeros(rows.shape[1:], F32)
    return np.cumsum(rows, axis=0, dtype=F32)[-1]


def twin(P, x, idx, val, norm, n_global=None, l1=0.0, slip=None, out=None, sparse_grads=False, ranged=None, list_perm=None):
    """The step behind the selection in float32, structured as csrc/sae.hip (prep, decode, gb_dec) and csrc/sae_bwd.hip (CSR by feature,
    chunk cuts, short walk, long lists in the token-range or the count-cut form, segment combine, zeroing of empty rows).  out: the
    gradient buffers to write into (what is not stored stays as it was; default: NaN).  ranged: force a segment form (default: the kernels' choice by n).
    list_perm: RandomState shuffling the pairs of the unsorted (count-cut) long lists, as the selection's atomics may.  slip: one of SLIPS."""
    assert slip is None or slip in SLIPS, slip
    P = {k_: np.asarray(v, F32) for k_, v in P.items()}
    x = np.asarray(x, F32)
    val = np.asarray(val, F32)
    idx = np.asarray(idx, np.int64)
    n, d = x.shape
    k = idx.shape[1]
    d_sae = P["W_dec"].shape[0]
    ng = n if n_global is None else n_global
    ranged = long_ranged(n) if ranged is None else ranged
    f = F32
    if O.norm_mode(norm) == "layer_norm":
        mu = (x.sum(axis=1, keepdims=True, dtype=F32) / f(d)).astype(F32)
        sq = ((x - mu) ** 2).sum(axis=1, keepdims=True, dtype=F32)
        sd = np.sqrt(sq / f(d - 1)).astype(F32)
        xh = (x - mu) / (sd + f(LN_EPS))
    else:
        mu, sd, xh = np.zeros((n, 1), F32), np.ones((n, 1), F32), x
    si = (xh - P["b_dec"]).astype(F32)
    bm = (x.sum(axis=0, keepdims=True, dtype=F32) * (f(1) / f(n))).astype(F32)
    nf = np.sqrt(((x - bm) ** 2).sum(axis=1, keepdims=True, dtype=F32)).astype(F32)
    live = (val != 0) if slip == "negative_value_live" else (val > 0)
    a = np.where(live, val, f(0)).astype(F32)
    acc = np.zeros((n, d), F32)
    for s in range(k):                                                        # slot order, as the decode kernel
        acc += a[:, s, None] * P["W_dec"][idx[:, s]]
    o = ((acc + P["b_dec"]) * sd + mu).astype(F32)
    e = (o - x).astype(F32)
    gs, ls = f(2.0) / (f(ng) * f(d)), f(1.0) / (f(ng) * f(d))
    loss = f(((e * e) / nf).sum(axis=1, dtype=F32).sum(dtype=F32) * ls)
    dY = (gs * e / nf * sd).astype(F32)
    dh = np.zeros((n, k), F32)
    for s in range(k):
        dh[:, s] = (dY * P["W_dec"][idx[:, s]]).sum(axis=1, dtype=F32)
    dh = np.where(live, dh + f(l1 / ng), f(0)).astype(F32)
    if l1:
        loss = f(loss + f(l1) * (a.sum(dtype=F32) / f(ng)))
    # CSR by feature: pair id p = token * k + slot, a list in ascending p = token order
    in_csr = np.ones_like(live) if slip == "holes_counted_and_filled" else live
    p_all = np.flatnonzero(in_csr.ravel())
    order = np.argsort(idx.ravel()[p_all], kind="stable")
    pairs = p_all[order]
    feat = idx.ravel()[pairs]
    counts = np.bincount(feat, minlength=d_sae)
    offs = np.concatenate([[0], np.cumsum(counts)])
    total = int(offs[-1])
    if out is None:
        out = dict(gW_dec=np.full((d_sae, d), np.nan, F32), gW_enc=np.full((d_sae, d), np.nan, F32), gb_enc=np.full(d_sae, np.nan, F32))
    gWd, gWe, gbe = out["gW_dec"], out["gW_enc"], out["gb_enc"]
    dcut = 256 * (d // 256) if (slip == "last_vector_dropped_at_ragged_d_in" and d % 256) else d
    vflat, dhflat = val.ravel(), dh.ravel()

    def terms(ps):
        tokn = ps % k if slip == "token_is_p_mod_k" else ps // k
        ap = vflat[np.minimum(ps + 1, vflat.size - 1)] if slip == "a_from_the_neighbouring_slot" else vflat[ps]
        gp = dhflat[ps]
        return (ap[:, None] * dY[tokn, :dcut]).astype(F32), (gp[:, None] * si[tokn, :dcut]).astype(F32), gp

    def walk(ps):
        td, te, gp = terms(ps)
        return _seqsum(td), _seqsum(te), _seqsum(gp)

    def store(j, gd, ge, gb):
        gWd[j, :dcut], gWe[j, :dcut], gbe[j] = gd, ge, gb

    lmax_walk = BWD_LMAX - 1 if slip == "list_of_64_owned_by_nobody" else BWD_LMAX       # the walk leaves lists of 64 to a long-list kernel
    lmax_reg = BWD_LMAX + 1 if slip == "list_of_65_through_the_64_lane_sort" else BWD_LMAX  # ... that registers only c > 64
    # chunk cuts: the grid point w * 16 that falls inside a list moves to that list's end (stays when it is the list's start)
    M = (total + BWD_CH - 1) // BWD_CH
    grid = np.arange(M) * BWD_CH
    jg = np.searchsorted(offs, grid, side="right") - 1
    cs = np.where(grid == offs[jg], grid, offs[np.minimum(jg + 1, d_sae)]) if M else np.zeros(0, np.int64)
    if slip == "chunk_cut_inside_a_list":
        cs = grid
    cs = np.concatenate([cs, [total]]).astype(np.int64)
    for w in range(M):
        q, q1 = int(cs[w]), int(cs[w + 1])
        while q < q1:
            j = int(feat[q])
            if counts[j] > lmax_walk:
                break                                                         # the long-list kernels own it
            qe = min(int(offs[j + 1]), q1)
            ps = pairs[q:qe]
            if slip == "list_of_65_through_the_64_lane_sort":
                ps = ps[:64]                                                  # the bitonic network holds 64 lanes
            store(j, *walk(ps))
            q = qe
    rs_tok = range_size(n)
    for j in np.flatnonzero(counts > lmax_reg):
        ps = pairs[offs[j]:offs[j + 1]]
        segs = []
        if ranged:
            tk = ps // k
            for r in range(BWD_RANGES):
                m = (tk >= r * rs_tok) & (tk < (r + 1) * rs_tok)
                if slip == "range_boundary_token_in_neither_range":
                    m &= ~((tk > 0) & (tk % rs_tok == 0))
                sp_ = ps[m]
                if slip == "segment_last_pair_dropped":
                    sp_ = sp_[:-1]
                per = (len(sp_) + SEG_WAVES - 1) // SEG_WAVES
                parts = [walk(sp_[min(w * per, len(sp_)):min(w * per + per, len(sp_))]) for w in range(SEG_WAVES)]
                segs.append(tuple(_seqsum(np.stack([pt[i] for pt in parts])) for i in range(3)))
        else:
            if list_perm is not None:
                ps = ps[list_perm.permutation(len(ps))]
            td, te, gp = terms(ps)
            for b in range(0, len(ps), BWD_SEG):
                hi = min(b + BWD_SEG, len(ps)) - (1 if slip == "segment_last_pair_dropped" else 0)
                segs.append((_seqsum(td[b:hi]), _seqsum(te[b:hi]), _seqsum(gp[b:hi])))
        if slip == "long_combine_stops_at_4_floor":
            segs = segs[:4 * (len(segs) // 4)]
        gd = _seqsum(np.stack([s_[0] for s_ in segs])) if segs else np.zeros(dcut, F32)
        ge = _seqsum(np.stack([s_[1] for s_ in segs])) if segs else np.zeros(dcut, F32)
        gb = f(0) if slip == "seg_b_not_summed_into_gb_enc" else (_seqsum(np.asarray([s_[2] for s_ in segs], F32)) if segs else f(0))
        store(j, gd, ge, gb)
    empty = counts == 0
    if sparse_grads:
        gbe[empty] = 0
    elif slip != "empty_rows_left_stale":
        gWd[empty], gWe[empty], gbe[empty] = 0, 0, 0
    gb_dec = (dY.sum(axis=0, dtype=F32) - (P["W_enc"] * gbe[None, :]).sum(axis=1, dtype=F32)).astype(F32)
    return dict(sae_out=o, loss=loss, l0=f(f(total) / f(n)), gW_dec=gWd, gW_enc=gWe, gb_enc=gbe, gb_dec=gb_dec,
                fire_count=counts.astype(F32), idx=idx, dY=dY, dh=dh)
