"""Planted inputs for the filtered top-k / ReLU encoder of csrc/sae_enc.hip: cases, float64 reference, per-element bounds, a numpy twin of
the filter's decisions, and the slips of the twin that the planted cases must catch.  numpy only.

Numbers, all derived from the code (sae.hpp, sae_enc.hip):
  N = 260 tokens: the filter GEMM's tile is 256 rows, so rows 256..259 live in a ragged second tile; the sample pass in its 128-row form
      (K % 64 == 0 and few tiles) puts them in its third tile.
  q = pv_sae_sample_q(k) = max(3 k / 8, 8): 8 at k = 8, 12 at k = 32, 24 at k = 64.
  slots = pv_sae_tile_slots: 4 * 16 * q / (d_sae / 256) + 6 rounded up to a power of two >= 16:
      (d_sae 2048, k 8) 70 -> 128;  (4096, 8) 38 -> 64;  (2048, 32) 102 -> 128;  (2048, 64) 198 -> 256.
      The one-round epilogue (ONE) runs where the K loop is the full-line form (d_in % 64 == 0) and slots <= 64: (64, 4096, 8) only.
      slots * (d_sae / 256) is 1024 = PV_SAE_CAND_CAP at k 8 and 32, so 1025 candidates without a slot overflow exist at k = 64 alone.
  HCAP = 8192 hits per compaction round in the full-line form (4096 otherwise); a round is the whole 256 x 256 tile in the ONE form.
  ns = d_sae / 16 sampled values: 128 at d_sae 2048 (two per lane of sae_thr_kernel<16>: the three-per-lane subset loses nothing),
      256 at 4096 (four per lane: a lane holding four of the top q gives a lower s_q).
  K loop: d_in 64 full-line, 96 pipelined, 40 / 264 / 1032 barrier-then-fetch; sae_select_kernel<1> up to d_in 256, <3> at 264, <5> at 1032.
  B_n = ||x|| (C1 Wmax + C2) + C2 Wmax + 4.8e-7 |v|, C1 = enc_c1(d_in) = 1.25e-3 up to d_in 916, 1.2843e-3 at 1032.

Grid rows: x has two nonzero entries, X_DN = 1 + 0.499 * 2^-10 (fp16: 1, the filter sees it 4.87e-4 too small) and X_UP = 1 + 0.501 * 2^-10
(fp16: 1 + 2^-10, 4.87e-4 too large), and every feature takes weight from at most one of the two rows of W_enc.  A filter value is then
fl32(fl16(x) fl16(w) + b) and an exact value fl32(fl32(x w) + b) in any summation order, so the twin predicts both bit for bit and with them
every decision of the filter.  (q = k at k = 8: s_q <= t always, so "all of the top-k in the sample" is decided with t == s_q there; it falls
back only where q < k.  A pre-activation of -0.0 cannot occur: the accumulators start at +0.0 and +0 + -0 = +0; the zeros row plants +0.0.)

Dense rows (``band_inversion``, the dense half of ``relu``): x = +-X_DN on the first half of d_in and +-X_UP on the second, winner columns
+-X_DN on the first half, loser columns +-X_UP on the second.  Every fp16 product is 1 or (1 + 2^-10)^2, their sums are exact in fp32, so the
filter value is still known exactly: the loser's is h (2^-9 + 2^-20) above the winner's (h = d_in / 2), 1.05 B_n, while the exact winner is
larger.  That is what the band 2 B_n is for; 1.1 B_n is all that operand rounding can reach on disjoint supports.

What the suite established: ``bias_dominated`` fails on the parent of this change (the twin's slip ``band_rounding_m_only``): B_n's rounding
term was scaled with |s_q| while the select kernel applies the band around t.  The select kernel now adds 9.6e-7 (|t| - |s_q|)."""
import functools

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -10                                           # fp16 spacing in [1, 2)
N_TOK = 260
STRIDE, CAND_CAP, RESCORE_MAX, RELU_SLOTS, SLOTS_MIN, MAXK = 16, 1024, 192, 32, 16, 64
GATE_MARGIN = 16.0
X_DN, X_UP = F32(1 + 0.499 * U), F32(1 + 0.501 * U)
BALLAST = 1                                              # the column that pins Wmax (b = -1e4: never near the top)
SLIPS = ("band_Bn", "c1_halved", "no_sq_check", "q_plus_1", "kth_no_multiplicity", "slots_ge", "no_overflow_mark",
         "rank_no_index_tiebreak", "relu_thr_zero", "band_rounding_m_only")


def fl16(v):
    with np.errstate(over="ignore"):
        return np.asarray(v, F32).astype(np.float16).astype(F32)


def sample_q(k):
    return max(k * 3 // 8, 8)


def tile_slots(d_sae, k):
    want = 4 * STRIDE * sample_q(k) // (d_sae // 256) + 6
    s = SLOTS_MIN
    while s < want:
        s *= 2
    return s


def loop_form(d_in):
    return 2 if d_in % 64 == 0 else (1 if d_in % 32 == 0 else 0)


def fast_ok(d_in, d_sae, k):
    return (d_sae % 256 == 0 and d_sae >= 2048 and d_in % 8 == 0 and d_in >= 32 and k <= MAXK and sample_q(k) * STRIDE * 2 <= CAND_CAP
            and tile_slots(d_sae, k) <= 256)


def enc_c1(d_in):
    return max(F32(1.25e-3), F32(F32(9.7680092e-4) + F32(F32(5.0) * F32(5.9604645e-8)) * F32(d_in)))


def band_B(xnorm, wmax, d_in, v, c1_scale=1.0):
    """B_n of the file header in fp32, with the rounding term at |v| (v = None: without it, as relu_thr_kernel)"""
    with np.errstate(invalid="ignore", over="ignore"):
        c1 = F32(enc_c1(d_in) * F32(c1_scale))
        c2 = F32(F32(2.98023224e-8) * np.sqrt(F32(d_in)))
        B = (np.asarray(xnorm, F32) * F32(c1 * wmax + c2) + F32(c2 * wmax)).astype(F32)
        if v is not None:
            B = (B + F32(4.8e-7) * np.abs(np.asarray(v, F32))).astype(F32)
    return B


class Case:
    def __init__(self, name, style, d_in, d_sae, k, W, b, x, labels, relu_cap=None, x2=None):
        assert relu_cap is not None or fast_ok(d_in, d_sae, k)
        self.name, self.style, self.d_in, self.d_sae, self.k = name, style, d_in, d_sae, k
        self.W, self.b, self.x, self.labels = W.astype(F32), b.astype(F32), x.astype(F32), labels
        self.n = x.shape[0]
        self.relu_cap, self.x2 = relu_cap, x2                 # (relu: x2 = the batch one token of which holds cap + 1 positives)
        self.slots = RELU_SLOTS if relu_cap else tile_slots(d_sae, k)
        self.q = sample_q(k)
        self.one_round = loop_form(d_in) == 2 and self.slots <= 64
        self.hcap = 8192 if loop_form(d_in) == 2 else 4096

    def where(self, j):
        """tile, wave column and lane that hold feature j in the filter GEMM's epilogue"""
        c = j % 256
        return f"feature {j} (tile {j // 256}, wave column {c // 64}, lane {c % 32}{'+32' if c % 64 >= 32 else ''})"


class Values:
    pass


@functools.lru_cache(maxsize=None)
def _values_cached(name, which):
    c = case(name)
    return values(c, c.x if which == 0 else c.x2)


def values(c, x=None, fast=False):
    """filter values a, exact values e (both fp32, as the kernels form them), float64 reference with its absolute sums, ||x||, Wmax.
    fast: fp32 products (the synthetic batches: no bit exactness wanted)"""
    x = c.x if x is None else x
    v = Values()
    T = F32 if fast else F64
    with np.errstate(over="ignore", invalid="ignore"):
        acc16 = fl16(x).astype(T) @ fl16(c.W).astype(T)
        acc = x.astype(T) @ c.W.astype(T)
        v.a = (acc16.astype(F32) + c.b[None]).astype(F32)
        v.e = (acc.astype(F32) + c.b[None]).astype(F32)
        v.grid_a = bool((acc16.astype(F32).astype(T) == acc16).all())
        v.ref = acc.astype(F64) + c.b[None].astype(F64)
        if not fast:
            v.S = np.abs(x).astype(F64) @ np.abs(c.W).astype(F64) + np.abs(c.b)[None].astype(F64)
        amax = np.abs(x).max(axis=1)
        v.xnorm = np.where(amax <= 6.0e4, np.sqrt((x.astype(F64) ** 2).sum(axis=1)), np.inf).astype(F32)
        colsq = (c.W.astype(F64) ** 2).sum(axis=0)
        colsq = np.where(np.abs(c.W).max(axis=0) > 65504, np.inf, colsq)
        v.wmax = F32(np.sqrt(colsq.max()))
    return v


def case_values(c, which=0):
    return _values_cached(c.name, which)


def value_bound(c, S):
    """re-scoring chain of sae_select_kernel / sae_fb_hidden_kernel: 4 ceil(d_in / 256) fmas per lane, 6 steps of the wave reduction, the bias
    add -- each rounds once, relative 2^-24 of a partial sum that |x|.|w| + |b| bounds; 1.001 for the second-order terms"""
    L = 4 * ((c.d_in + 255) // 256)
    return (L + 6 + 1) * 2.0 ** -24 * 1.001 * S + 2.0 ** -126


def reference(c, which=0):
    """top-k of the float64 pre-activations: order (value descending, index ascending); tie[n]: ranks k and k + 1 are equal"""
    v = case_values(c, which)
    order = np.lexsort((np.broadcast_to(np.arange(c.d_sae), v.ref.shape), -v.ref), axis=1)
    idx = order[:, :c.k]
    nxt = order[:, c.k]
    rows = np.arange(c.n)
    kth, kth1 = v.ref[rows, idx[:, -1]], v.ref[rows, nxt]
    bound = np.maximum(value_bound(c, v.S[rows, idx[:, -1]]), value_bound(c, v.S[rows, nxt]))
    return dict(idx=idx, val=np.maximum(np.take_along_axis(v.ref, idx, 1), 0), tie=kth == kth1, gap=(kth - kth1) / bound, ref=v.ref, S=v.S,
                positive=v.ref > 0)


# ---------------------------------------------------------------------------------------------------
# the twin
# ---------------------------------------------------------------------------------------------------
def _sq(a, q):
    """sae_thr_kernel: every lane's three largest of the sampled values it holds (column c of the sample in lane c % 64), then the q-th
    largest of those with multiplicity"""
    samp = a[:, ::STRIDE].copy()
    samp[samp != samp] = -np.inf
    n, ns = samp.shape
    pad = (-ns) % 64
    if pad:
        samp = np.concatenate([samp, np.full((n, pad), -np.inf, F32)], axis=1)
    V = np.sort(samp.reshape(n, -1, 64), axis=1)[:, -3:, :].reshape(n, -1)
    if V.shape[1] < q:
        return np.full(n, -np.inf, F32)
    return np.sort(V, axis=1)[:, -q]


def exact_topk(e_row, k):
    order = np.lexsort((np.arange(e_row.size), -e_row))[:k]
    return order, np.maximum(e_row[order], F32(0))


def twin(c, slip=None, v=None):
    """index lists, values and outcome of every token as sae_encode_fast forms them.  outcome: "decided", or why the token takes the exact
    path ("slots", "hcap?", "count", "t<sq", "band"); "hcap?": the block's hits passed HCAP, which rows were marked depends on wave order"""
    assert slip is None or slip in SLIPS
    v = case_values(c) if v is None else v
    a, e, k, n = v.a, v.e, c.k, v.a.shape[0]
    ntn = c.d_sae // 256
    q = c.q + (1 if slip == "q_plus_1" else 0)
    sq = _sq(a, q)
    B = band_B(v.xnorm, v.wmax, c.d_in, sq, 0.5 if slip == "c1_halved" else 1.0)
    band = B if slip == "band_Bn" else (F32(2) * B).astype(F32)
    with np.errstate(invalid="ignore"):
        thr = (sq - band).astype(F32)
        hits = a >= thr[:, None]
    per_tile = hits.reshape(n, ntn, 256).sum(axis=2)
    rows = np.arange(n)
    grp = rows // 256 if c.one_round else (rows // 256) * 4 + (rows % 128) // 32
    hc = np.zeros((grp.max() + 1, ntn), np.int64)
    np.add.at(hc, grp, per_tile)
    hcap_hit = (hc[grp] > c.hcap) & (per_tile > 0)
    out = dict(idx=np.full((n, k), -1, np.int64), val=np.zeros((n, k), F32), outcome=[], ncand=hits.sum(axis=1), nr=np.zeros(n, np.int64),
               t=np.full(n, np.nan, F32), sq=sq, B=B, thr=thr)
    for r in range(n):
        cols = np.flatnonzero(hits[r])
        av = a[r, cols]
        why = None
        over = per_tile[r] >= c.slots if slip == "slots_ge" else per_tile[r] > c.slots
        if hcap_hit[r].any() and slip != "no_overflow_mark":
            why = "hcap?"
        elif over.any() or hcap_hit[r].any():
            if slip == "no_overflow_mark":                    # the list is cut at `slots` and nobody is told: the largest are gone
                keep = np.ones(cols.size, bool)
                for tl in np.flatnonzero(per_tile[r] > c.slots):
                    m = np.flatnonzero(cols // 256 == tl)
                    keep[m[np.argsort(av[m], kind="stable")[c.slots:]]] = False
                cols, av = cols[keep], av[keep]
            else:
                why = "slots"
        if why is None and (cols.size > CAND_CAP or cols.size < k or not np.isfinite(B[r])):
            why = "count"
        if why is None:
            if slip == "kth_no_multiplicity":
                uq = np.unique(av)
                t = uq[-k] if uq.size >= k else uq[0]
            else:
                t = np.sort(av)[-k]
            out["t"][r] = t
            if not t >= sq[r] and slip != "no_sq_check":
                why = "t<sq"
        if why is None:
            extra = F32(0) if slip == "band_rounding_m_only" else F32(9.6e-7) * max(F32(abs(t)) - F32(abs(sq[r])), F32(0))
            lo = F32(t - F32(band[r] + extra))
            inb = av >= lo
            out["nr"][r] = inb.sum()
            if inb.sum() > RESCORE_MAX:
                why = "band"
        if why is None:
            ci, ev = cols[inb], e[r, cols[inb]]
            if slip == "rank_no_index_tiebreak":              # tied entries draw the same rank: one slot written twice, one never
                rank = (ev[None, :] > ev[:, None]).sum(axis=1)
                for p in range(ci.size):
                    if rank[p] < k:
                        out["idx"][r, rank[p]], out["val"][r, rank[p]] = ci[p], max(ev[p], F32(0))
            else:
                o = np.lexsort((ci, -ev))[:k]
                out["idx"][r, :o.size], out["val"][r, :o.size] = ci[o], np.maximum(ev[o], F32(0))
            why = "decided"
        else:
            out["idx"][r], out["val"][r] = exact_topk(e[r], k)
        out["outcome"].append(why)
    out["fallbacks"] = sum(w != "decided" for w in out["outcome"])
    return out


def twin_relu(c, slip=None, which=0):
    """relu_thr_kernel / the ReLU filter / relu_select_kernel: per-token lists of the positive exact values among the features whose filter
    value is >= -B_n, (value descending, index ascending); mode 1 where a token cannot be held"""
    v = case_values(c, which)
    a, e, n, cap = v.a, v.e, v.a.shape[0], c.relu_cap
    B = band_B(v.xnorm, v.wmax, c.d_in, None, 0.5 if slip == "c1_halved" else 1.0)
    thr = np.zeros(n, F32) if slip == "relu_thr_zero" else -B
    hits = a >= thr[:, None]
    per_tile = hits.reshape(n, c.d_sae // 256, 256).sum(axis=2)
    mode = int((per_tile > RELU_SLOTS).any() or (hits.sum(axis=1) > CAND_CAP).any())
    lists = []
    for r in range(n):
        cols = np.flatnonzero(hits[r])
        ev = e[r, cols]
        pos = ev > 0
        if (a[r, cols] > B[r]).sum() > cap or pos.sum() > cap:
            mode = 1
        o = np.lexsort((cols[pos], -ev[pos]))
        lists.append((cols[pos][o], ev[pos][o]))
    return dict(mode=mode, lists=lists, B=B, ncand=hits.sum(axis=1))


# ---------------------------------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------------------------------
def check(c, got, which=0):
    """got = dict(idx [n, k], val [n, k]) -> (worst error / bound, messages).  Index sets must be the reference's; on a tie at rank k: k distinct
    indices, every kept value >= every dropped one (to within the bound), values those of the reference's multiset."""
    r = reference(c, which)
    worst, msgs = 0.0, []
    for n in range(c.n):
        gi, gv = np.asarray(got["idx"][n]).astype(np.int64), np.asarray(got["val"][n], F64)
        label = f"token {n} ({c.labels[n]})"
        if len(set(gi.tolist())) != c.k or gi.min() < 0 or gi.max() >= c.d_sae:
            msgs.append(f"{label}: indices {gi.tolist()} are not k distinct features")
            worst = np.inf
            continue
        bnd = value_bound(c, r["S"][n, gi])
        ratio = np.abs(gv - np.maximum(r["ref"][n, gi], 0)) / bnd
        if ratio.max() > 1:
            j = gi[ratio.argmax()]
            msgs.append(f"{label}: value of {c.where(j)} is {gv[ratio.argmax()]!r}, reference {max(r['ref'][n, j], 0)!r}: {ratio.max():.3g} bounds")
        worst = max(worst, float(ratio.max()))
        if not r["tie"][n]:
            if set(gi.tolist()) != set(r["idx"][n].tolist()):
                lost = sorted(set(r["idx"][n].tolist()) - set(gi.tolist()))
                extra = sorted(set(gi.tolist()) - set(r["idx"][n].tolist()))
                msgs.append(f"{label}: lost {', '.join(c.where(j) for j in lost)}; kept instead {extra}")
                worst = np.inf
        else:
            dropped = np.ones(c.d_sae, bool)
            dropped[gi] = False
            if r["ref"][n, gi].min() < r["ref"][n, dropped].max() or not np.array_equal(np.sort(r["ref"][n, gi]), np.sort(r["ref"][n, r["idx"][n]])):
                msgs.append(f"{label}: kept values are not the k largest of a tied row")
                worst = np.inf
    return worst, msgs


def check_relu(c, got, which=0):
    """got = dict(idx [n, cap], val [n, cap], count [n]) of a step that ran sparse"""
    r = reference(c, which)
    worst, msgs = 0.0, []
    for n in range(c.n):
        m = int(got["count"][n])
        gi, gv = np.asarray(got["idx"][n][:m]).astype(np.int64), np.asarray(got["val"][n][:m], F64)
        want = np.flatnonzero(r["positive"][n])
        label = f"token {n} ({c.labels[n]})"
        if sorted(gi.tolist()) != want.tolist():
            lost, extra = sorted(set(want.tolist()) - set(gi.tolist())), sorted(set(gi.tolist()) - set(want.tolist()))
            msgs.append(f"{label}: lost {', '.join(c.where(j) for j in lost)}; listed without being positive {', '.join(c.where(j) for j in extra)}")
            worst = np.inf
            continue
        if m:
            ratio = np.abs(gv - r["ref"][n, gi]) / value_bound(c, r["S"][n, gi])
            worst = max(worst, float(ratio.max()))
            if ratio.max() > 1:
                msgs.append(f"{label}: value of {c.where(gi[ratio.argmax()])}: {ratio.max():.3g} bounds")
    return worst, msgs


def relu_margin(c, which=0):
    """smallest |pre-activation| / bound over the batch, exact zeros aside (they must not be listed and cannot be mistaken: see the module
    docstring of the CPU test)"""
    v = case_values(c, which)
    nz = v.ref != 0
    return float((np.abs(v.ref[nz]) / value_bound(c, v.S[nz])).min())


# ---------------------------------------------------------------------------------------------------
# grid cases: scenes of planted (column, weight) lists, two input dimensions each
# ---------------------------------------------------------------------------------------------------
class Grid:
    def __init__(self, d_in, d_sae, k, pairs=None, ballast=16.0, bias=0.0):
        self.d_in, self.d_sae, self.k, self.q = d_in, d_sae, k, sample_q(k)
        self.W, self.b = np.zeros((d_in, d_sae), F32), np.full(d_sae, bias, F32)
        self.pairs = pairs or [(2 * s, 2 * s + 1) for s in range(d_in // 2)]
        self.labels, self.ballast = [], ballast
        if ballast:
            self.W[self.pairs[0][0], BALLAST], self.b[BALLAST] = ballast, -1.0e4
        self.forced, self.rare = {}, set()                      # rare: scenes that only forced tokens take

    def cols(self, on_sample, count, tiles=None, skip=()):
        """`count` unused columns on (j % 16 == 0) or off the sample, taken round-robin from `tiles`"""
        tiles = list(range(self.d_sae // 256)) if tiles is None else list(tiles)
        per = {t: [j for j in range(t * 256, t * 256 + 256) if (j % 16 == 0) == on_sample and j != BALLAST and j not in self._used and j not in skip]
               for t in tiles}
        got, i = [], 0
        while len(got) < count:
            t = tiles[i % len(tiles)]
            i += 1
            if per[t]:
                got.append(per[t].pop(0))
            assert any(per.values()) or len(got) == count, "out of columns"
        self._used.update(got)
        return np.asarray(got)

    def scene(self, label):
        self.labels.append(label)
        self._used = set()
        return len(self.labels) - 1

    def plant(self, s, cols, vals, side=0):
        cols = np.asarray(cols)
        self._used.update(cols.tolist())
        assert (self.W[self.pairs[s][1 - side], cols] == 0).all(), "a feature takes weight from one of the scene's two rows only"
        self.W[self.pairs[s][side], cols] = np.asarray(vals, F32)

    def anchors(self, s, level, count=None, tiles=None, step=2 * U):
        """`count` (q) sampled columns from `level` down: they set s_q"""
        count = self.q if count is None else count
        self.plant(s, self.cols(True, count, tiles), level - step * np.arange(count))

    def force(self, token, s):
        self.forced[token] = s

    def build(self, name, style="grid", relu_cap=None, n=N_TOK):
        S = len(self.labels)
        assert S <= len(self.pairs)
        common = [s for s in range(S) if s not in self.rare]
        scene_of = [self.forced.get(t, common[t % len(common)]) for t in range(n)]
        x = np.zeros((n, self.d_in), F32)
        for t, s in enumerate(scene_of):
            x[t, self.pairs[s][0]], x[t, self.pairs[s][1]] = X_DN, X_UP
        if self.ballast:
            norms = np.sqrt((self.W.astype(F64) ** 2).sum(axis=0))
            assert np.delete(norms, BALLAST).max() < self.ballast and norms[BALLAST] == self.ballast
        return Case(name, style, self.d_in, self.d_sae, self.k, self.W, self.b, x, [self.labels[s] for s in scene_of], relu_cap=relu_cap)


def _plain(g, label, winners_tiles=None, on_sample=False, top=1.9, anchor=1.2, losers=4):
    """k winners from `top` down in steps of 2^-9, a few losers 0.02 below the last, q sampled anchors at `anchor`: decided"""
    s = g.scene(label)
    g.plant(s, g.cols(on_sample, g.k, winners_tiles), top - 2 * U * np.arange(g.k), side=0)
    g.plant(s, g.cols(False, losers), top - 2 * U * g.k - 0.02 - 2 * U * np.arange(losers), side=1)      # (inside the band at k = 8)
    g.anchors(s, anchor)
    return s


def _edges():
    """(64, 2048, 8): slots 128, a compaction round per 64-row block"""
    g = Grid(64, 2048, 8)
    _plain(g, "none_in_sample")
    s = g.scene("all_in_sample: t == s_q, decided")                               # (q == k)
    g.plant(s, g.cols(True, 8), 1.9 - 2 * U * np.arange(8))
    g.plant(s, g.cols(True, 8), 1.7 - 2 * U * np.arange(8), side=1)
    # tile_edges: all k winners in one tile, at its first and last column and both sides of every 32- and 64-column boundary
    for tl, name in ((0, "first"), (7, "last")):
        s = g.scene(f"tile_edges: winners in the {name} tile")
        base = tl * 256
        g.plant(s, base + np.asarray([0, 31, 32, 63, 64, 127, 128, 255]), 1.9 - 2 * U * np.arange(8))
        g.plant(s, base + np.asarray([2, 33, 65, 95, 97, 129, 191, 193, 254]), 1.8 - 2 * U * np.arange(9), side=1)
        g.anchors(s, 1.2, tiles=[3, 4])
    s = g.scene("tile_edges: winners at 0, 255, 256 and d_sae - 1")
    g.plant(s, [0, 255, 256, 2047, 511, 512, 1791, 1792], 1.9 - 2 * U * np.arange(8))
    g.plant(s, [254, 257, 2046, 510, 513], 1.8 - 2 * U * np.arange(5), side=1)
    g.anchors(s, 1.2)
    # slot_edges: a (token, tile) list of exactly `slots` hits, and one more
    for extra in (0, 1):
        s = g.scene(f"slot_edges: {128 + extra} hits in tile 2")
        g.plant(s, g.cols(False, 8, [2]), 1.9 - 2 * U * np.arange(8))
        g.plant(s, g.cols(False, 112 + extra, [2]), 1.5 - 0.25 * U * np.arange(112 + extra), side=1)
        g.anchors(s, 1.2, tiles=[2])                                                 # (8 more hits in tile 2: 128 / 129)
    # candidate_counts: 255 / 256 / 257 (register select / LDS select), 1024 (the list's capacity, every tile full)
    for total in (255, 256, 257, 1024):
        s = g.scene(f"candidate_counts: {total} candidates")
        g.plant(s, g.cols(False, 8), 1.9 - 2 * U * np.arange(8))
        g.anchors(s, 1.2)
        rest = total - 16
        g.plant(s, g.cols(False, rest), 1.6 - 0.375 * np.arange(rest) / rest, side=1)   # (all above thr = s_q - 2 B_n = 1.13)
    # band_population: 192 / 193 candidates within the band below t (PV_SAE_RESCORE_MAX)
    for total in (192, 193):
        s = g.scene(f"band_population: {total} within the band")
        g.plant(s, g.cols(False, 8), 1.9 - 2 * U * np.arange(8))
        g.plant(s, g.cols(False, total - 8), 1.9 - 18 * U - 0.0125 * np.arange(total - 8) / (total - 8), side=1)
        g.plant(s, g.cols(False, 40), 1.7 - 2 * U * np.arange(40), side=1)        # candidates outside the band
        g.anchors(s, 1.2)
    # repeated_keys: filter values equal in a run that straddles rank k; their exact values differ (weights within one fp16 step)
    s = g.scene("repeated_keys: five equal filter values at ranks 6..10")
    g.plant(s, g.cols(False, 5), 1.9 - 2 * U * np.arange(5))
    run = g.cols(False, 5)
    g.plant(s, run, fl16(1.85) + U * np.asarray([0.1, 0.4, -0.3, 0.25, -0.1]))     # fl16 of each is fl16(1.85)
    g.plant(s, g.cols(False, 3), 1.8 - 2 * U * np.arange(3), side=1)
    g.anchors(s, 1.2)
    s = g.scene("repeated_keys: exact ties across rank k after re-scoring")
    g.plant(s, g.cols(False, 6), 1.9 - 2 * U * np.arange(6))
    g.plant(s, [1500, 700, 1100, 300], fl16(1.85) * np.ones(4))                      # 4-way exact tie at ranks 7..10: 300 and 700 are kept
    g.anchors(s, 1.2)
    s = g.scene("repeated_keys: a run above rank k, distinct k-th below s_q")
    g.plant(s, g.cols(False, 6), fl16(1.9) * np.ones(6) + U * 0.05 * np.arange(6))  # six equal filter values
    g.plant(s, g.cols(False, 2), [1.85, 1.84])                                        # t = 1.84 counts multiplicity: ranks 7, 8
    g.plant(s, g.cols(True, 8), fl16(1.8) * np.ones(8))                               # s_q = 1.8 eight times over
    g.plant(s, g.cols(False, 5), 1.79 - 2 * U * np.arange(5), side=1)                 # the 8th DISTINCT value lies among these, below s_q
    s = g.scene("zeros: six positives, every other pre-activation +0.0")             # s_q = 0: everything is a hit, the slots overflow
    g.plant(s, g.cols(False, 6), 1.9 - 2 * U * np.arange(6))
    for t, sc in ((0, 2), (31, 3), (32, 4), (255, 2), (256, 3), (259, 4)):            # tile_edges in the first and last rows of both row tiles
        g.force(t, sc)
    return g.build("edges")


def _one_round():
    """(64, 4096, 8): slots 64 and the ONE epilogue; four sampled values per lane of sae_thr_kernel"""
    g = Grid(64, 4096, 8)
    _plain(g, "none_in_sample")
    s = g.scene("one_lane: the four largest sampled values in lane 5")
    g.plant(s, g.cols(False, 8), 1.9 - 2 * U * np.arange(8))
    g.plant(s, 16 * np.asarray([5, 69, 133, 197]), [1.5, 1.49, 1.48, 1.47])
    g.plant(s, 16 * np.asarray([6, 71, 136, 201, 10, 75, 140, 205]), 1.3 - 2 * U * np.arange(8))
    g.plant(s, g.cols(False, 6), 1.29 - 2 * U * np.arange(6), side=1)                 # hits either way; s_q is 1.3 - 8 U, not 1.3 - 6 U
    for extra in (0, 1):
        s = g.scene(f"slot_edges: {64 + extra} hits in tile 15")
        g.plant(s, g.cols(False, 8, [15]), 1.9 - 2 * U * np.arange(8))
        g.plant(s, g.cols(False, 48 + extra, [15]), 1.5 - 0.25 * U * np.arange(48 + extra), side=1)
        g.anchors(s, 1.2, tiles=[15])
    s = g.scene("tile_edges: winners at 0, 255, 256 and d_sae - 1")
    g.plant(s, [0, 255, 256, 4095, 3839, 3840, 2047, 2048], 1.9 - 2 * U * np.arange(8))
    g.plant(s, [254, 257, 4094, 3838, 3841], 1.8 - 2 * U * np.arange(5), side=1)
    g.anchors(s, 1.2)
    for t, sc in ((0, 4), (31, 1), (32, 4), (255, 1), (256, 4), (259, 1)):
        g.force(t, sc)
    return g.build("one_round")


def _hcap():
    """(64, 4096, 8), the ONE epilogue: every token has 40 hits in tile 3 (below its 64 slots), the 256-row tile 10 240 (above HCAP = 8192);
    the 4 rows of the ragged tile have 160"""
    g = Grid(64, 4096, 8)
    s = g.scene("slot_edges: the tile's hits pass HCAP")
    g.plant(s, g.cols(False, 8, [3]), 1.9 - 2 * U * np.arange(8))
    g.plant(s, g.cols(False, 24, [3]), 1.5 - 2 * U * np.arange(24), side=1)
    g.anchors(s, 1.2, tiles=[3])
    return g.build("hcap")


def _k32():
    """(96, 2048, 32): q = 12 < k; the pipelined K loop"""
    g = Grid(96, 2048, 32)
    _plain(g, "none_in_sample")
    s = g.scene("all_in_sample: s_q above t, too few candidates")
    g.plant(s, g.cols(True, 32), 1.9 - 6 * U * np.arange(32))
    g.plant(s, g.cols(False, 4), 1.6 - 2 * U * np.arange(4), side=1)
    s = g.scene("all_in_sample: s_q above t, k candidates")
    g.plant(s, g.cols(True, 32), 1.9 - 0.25 * U * np.arange(32))
    g.plant(s, g.cols(False, 4), 1.7 - 2 * U * np.arange(4), side=1)
    s = g.scene("sample: t between s_q and s_(q+1)")
    g.plant(s, g.cols(True, 12), 1.9 - 0.25 * U * np.arange(12))
    g.plant(s, g.cols(True, 6), 1.5 - 2 * U * np.arange(6))
    g.plant(s, g.cols(False, 25), 1.8 - 0.25 * U * np.arange(25), side=1)
    s = g.scene("sq_gate: t just above the threshold, a top-k feature just below it")
    V0 = fl16(1.9)
    g.plant(s, g.cols(True, 12), V0 * np.ones(12) + 0.04 * U * np.arange(12))
    g.plant(s, g.cols(False, 19), V0 * np.ones(19) + 0.02 * U * np.arange(19))
    cT, cU = g.cols(False, 2)
    # thr = V0 - 2 B_n is no fp16 value.  U (first row: the filter sees it low) gets the largest fp16 weight gU below thr, T (second row:
    # seen high) gT = gU - 2^-10: a_T = gT (1 + 2^-10) must still reach thr, while exactly e_U > e_T.
    xn = F32(np.sqrt(F64(X_DN) ** 2 + F64(X_UP) ** 2))
    thr = F32(V0 - F32(2) * band_B(xn, F32(g.ballast), 96, V0))
    gU = fl16(thr)
    gU = gU if gU < thr else F32(gU - U)
    gT = F32(gU - U)
    assert gT * F32(1 + U) >= thr + 1e-5 and gU <= thr - 1e-5, (gT * F32(1 + U) - thr, thr - gU)
    g.plant(s, [cU], [gU], side=0)
    g.plant(s, [cT], [gT], side=1)
    return g.build("k32")


def _k64():
    """(40, 2048, 64): q = 24, slots 256; barrier-then-fetch K loop with a K tail, lane columns beyond d_in masked; the scenes sit on the last
    input dimensions"""
    g = Grid(40, 2048, 64, pairs=[(38, 39), (36, 37), (0, 1), (2, 3), (34, 35)])
    _plain(g, "none_in_sample")
    for total in (1024, 1025):
        s = g.scene(f"candidate_counts: {total} candidates")
        g.plant(s, g.cols(False, 64), 1.9 - 0.5 * U * np.arange(64))
        g.anchors(s, 1.2, step=0.5 * U)
        rest = total - 64 - 24
        g.plant(s, g.cols(False, rest), 1.6 - 0.375 * np.arange(rest) / rest, side=1)
        g.rare.add(s)                                            # (a 64-row round holds 4096 hits per tile: three such tokens, apart)
        for t in ((5, 200, 257) if total == 1024 else (6, 130, 258)):
            g.force(t, s)
    s = g.scene("candidate_counts: fewer than k candidates")
    g.plant(s, g.cols(True, 24), 1.9 - 2 * U * np.arange(24))
    g.plant(s, g.cols(False, 50), 1.5 - 2 * U * np.arange(50), side=1)
    return g.build("k64")


def _wide(d_in):
    """d_in 264 / 1032: sae_select_kernel<3> / <5> with the last lane columns masked, K tails in the filter GEMM; scenes on the last dimensions"""
    g = Grid(d_in, 2048, 8, pairs=[(d_in - 2, d_in - 1), (d_in - 8, d_in - 5), (0, 255), (3, d_in - 3)])
    _plain(g, "none_in_sample")
    s = g.scene("tile_edges: winners at 0, 255, 256 and d_sae - 1")
    g.plant(s, [0, 255, 256, 2047, 511, 512, 1791, 1792], 1.9 - 2 * U * np.arange(8))
    g.plant(s, [254, 257, 2046, 510, 513], 1.8 - 2 * U * np.arange(5), side=1)
    g.anchors(s, 1.2)
    s = g.scene("all_in_sample: t == s_q, decided")
    g.plant(s, g.cols(True, 8), 1.9 - 2 * U * np.arange(8))
    g.plant(s, g.cols(True, 8), 1.7 - 2 * U * np.arange(8), side=1)
    s = g.scene("slot_edges: 129 hits in tile 5")
    g.plant(s, g.cols(False, 8, [5]), 1.9 - 2 * U * np.arange(8))
    g.plant(s, g.cols(False, 113, [5]), 1.5 - 0.25 * U * np.arange(113), side=1)
    g.anchors(s, 1.2, tiles=[5])
    return g.build(f"d{d_in}")


def _negative():
    """every pre-activation negative (b_enc = -16 everywhere): ordered keys of negative floats; kept values are exactly 0 (the row of +0.0
    around rank k is the zeros scene of ``edges``)"""
    g = Grid(64, 2048, 8, bias=-16.0)
    for name, on in (("none_in_sample", False), ("all_in_sample", True)):
        s = g.scene(f"negative_rows: {name}")
        g.plant(s, g.cols(on, 8), 1.9 - 2 * U * np.arange(8))
        g.plant(s, g.cols(False, 5), 1.8 - 2 * U * np.arange(5), side=1)
        g.anchors(s, 1.2)
    c = g.build("negative")
    return c


# ---------------------------------------------------------------------------------------------------
# dense rounding-adversarial rows
# ---------------------------------------------------------------------------------------------------
def _dense_parts(d_in, d_sae, rs, lo, hi):
    """signs, x, and the column makers of a dense scene on the input dimensions [lo, hi): first half seen low, second half seen high"""
    h = (hi - lo) // 2
    sg = rs.choice([-1.0, 1.0], size=hi - lo).astype(F32)
    x = np.zeros(d_in, F32)
    x[lo:lo + h], x[lo + h:hi] = sg[:h] * X_DN, sg[h:] * X_UP

    def winner(tweak_dim, tweak):
        w = np.zeros(d_in, F32)
        w[lo:lo + h] = sg[:h] * X_DN
        w[lo + tweak_dim] = sg[tweak_dim] * F32(1 + tweak * U)             # an fp16 value: this weight does not round
        return w

    def loser(scale=1.0):
        w = np.zeros(d_in, F32)
        w[lo + h:hi] = sg[h:] * X_UP * F32(scale)
        return w

    return h, x, winner, loser


def _band_inversion(d_in):
    """k winners on the first half of x, k + 2 losers on the second; tokens differ by a power of two.  tweak: one weight of each winner is
    (1 + tweak 2^-10), which lifts its exact value GATE_MARGIN bounds and more above the losers' while the filter still sees it more than
    B_n below"""
    d_sae, k = 2048, 8
    rs = np.random.RandomState(d_in)
    h, x0, winner, loser = _dense_parts(d_in, d_sae, rs, 0, d_in)
    tweak = 3 if d_in == 64 else 24
    W, b = np.zeros((d_in, d_sae), F32), np.zeros(d_sae, F32)
    off = [j for j in range(d_sae) if j % 16][5::7]
    win, lose = off[:k], off[100:100 + k + 2]
    for i, j in enumerate(win):
        W[:, j] = winner(i, tweak)
    for j in lose:
        W[:, j] = loser()
    for i, j in enumerate(range(16, 16 + 16 * sample_q(k), 16)):                       # q sampled anchors at half the size
        W[:, j] = loser(0.5 - i / 64.0)
    x = np.stack([x0 * F32(2.0 ** (t % 5 - 2)) for t in range(N_TOK)])
    c = Case(f"band_inversion_{d_in}", "dense", d_in, d_sae, k, W, b, x, [f"band_inversion: scale 2^{t % 5 - 2}" for t in range(N_TOK)])
    c.winners, c.losers = np.asarray(win), np.asarray(lose)
    return c


def _relu():
    """(64, 2048), cap 8.  Input dimensions 0..31: dense rows (b_enc makes the planted features cross zero); 32..63: grid scenes.
    b_enc = -1 elsewhere, so a feature no scene plants is -1 and never a candidate."""
    d_in, d_sae, cap = 64, 2048, 8
    g = Grid(d_in, d_sae, 8, pairs=[(32 + 2 * s, 33 + 2 * s) for s in range(16)], ballast=None, bias=-1.0)
    rs = np.random.RandomState(7)
    h, x0, winner, loser = _dense_parts(d_in, d_sae, rs, 0, 32)
    ev = lambda w: float(x0.astype(F64) @ w.astype(F64))                                # noqa: E731
    # dense: exact +2^-11 with the filter value -0.53 B_n (must be listed); the mirror (must not); a plain positive
    ww, wl = winner(0, 0), loser()
    cols = dict(pos_seen_negative=40, neg_seen_positive=41, plain=42)
    g.W[:, 40], g.b[40] = ww, F32(-(ev(ww) - 2.0 ** -11))
    g.W[:, 41], g.b[41] = wl, F32(-(ev(wl) + 2.0 ** -11))
    g.W[:, 42], g.b[42] = wl, F32(-(ev(wl) - 1.0))
    # grid scenes (weights 1 + ...: b = -1)
    s = g.scene("relu_zero_crossing: exact zero, small positives and negatives")
    g.plant(s, [300], [1.0], side=0)              # exact +4.87e-4, filter value exactly 0: listed
    g.plant(s, [301], [F32(1 - U)], side=1)        # exact -4.9e-4, filter value -2^-20 (a candidate): not listed
    g.plant(s, [302, 303], [1.5, 1.25], side=0)
    g.b[304] = 0.0                                  # pre-activation exactly 0 in every scene: never listed
    for m in (cap, cap - 1):
        s = g.scene(f"relu_zero_crossing: {m} positives")
        g.plant(s, g.cols(False, m, skip=(300, 301, 302, 303, 304, 40, 41, 42)), 1.5 + 0.01 * np.arange(m), side=0)
    c = g.build("relu", relu_cap=cap)
    # tokens 3 (mod 4): the dense row
    for t in range(3, N_TOK, 4):
        c.x[t] = x0
        c.labels[t] = "relu_zero_crossing: dense row"
    c.dense_cols = cols
    # the second batch: token 258 (scene of cap - 1 positives ... ) replaced by a row with cap + 1
    x2 = c.x.copy()
    s9 = len(g.labels)
    dn, up = g.pairs[s9]
    c.W[dn, 600:600 + cap + 1] = 1.5 + 0.01 * np.arange(cap + 1)
    x2[258] = 0
    x2[258, dn], x2[258, up] = X_DN, X_UP
    c.x2 = x2
    return c


CASES = ("edges", "one_round", "hcap", "k32", "k64", "d264", "d1032", "negative", "bias_dominated_20", "bias_dominated_10",
         "bias_dominated_4", "band_inversion_64", "band_inversion_1032")
RELU_CASES = ("relu",)


def _bias_ratio_case(r):
    """nine features with b_enc = 2^p, off the sample.  Eight take 0.0624625 * 2^(p - 20) from the row the filter sees high (X_UP): the sum
    rounds up to 2^p + one fp32 step in the filter and down to 2^p exactly.  One, C, takes 0.0625 * 2^(p - 20) from the row it sees low: the
    reverse.  Exactly, C is the largest value of the row; in the filter it lies one fp32 step of 2^p below t.  The sampled anchors sit at
    2^(p - r), so t / |s_q| = 2^r.  r = 20 (p = 20, anchors at 1): the row of the issue -- the step, 0.125, is 300 times the band where its
    rounding term is scaled with |s_q|.  r = 10 (p = 20) and r = 4 (p = 14): anchors at 1024, whose band covers the step either way."""
    p = 20 if r >= 10 else 14
    sc = 2.0 ** (p - 20)
    g = Grid(64, 2048, 8, ballast=None)
    for label in ("bias_dominated", "bias_dominated, a second pair of rows"):
        s = g.scene(f"{label}: t / |s_q| = 2^{r}")
        if s == 0:
            eight, C = g.cols(False, 8), g.cols(False, 1)
        g.plant(s, eight, 0.0624625 * sc * np.ones(8), side=1)
        g.plant(s, C, [0.0625 * sc], side=0)
        lvl = 2.0 ** (p - r)
        g.anchors(s, lvl, step=2 * U * lvl)
    g.b[np.concatenate([eight, C])] = 2.0 ** p
    c = g.build(f"bias_dominated_{r}")
    c.eight, c.C = eight, int(C[0])
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    if name.startswith("bias_dominated_"):
        return _bias_ratio_case(int(name.rsplit("_", 1)[1]))
    if name.startswith("band_inversion_"):
        return _band_inversion(int(name.rsplit("_", 1)[1]))
    if name in ("d264", "d1032"):
        return _wide(int(name[1:]))
    return {"edges": _edges, "one_round": _one_round, "hcap": _hcap, "k32": _k32, "k64": _k64, "negative": _negative, "relu": _relu}[name]()
