"""Planted operand ranges for the dense SAE steps of csrc/sae_dense.hip and csrc/sae_gated.hip on the GEMM of csrc/sae_dense_gemm.hip
(the ReLU + L1 step, its tanh-relu / lp_norm > 1 tail, the gated
step), a float64 reference with the absolute sums a bound needs, per-element bounds for both forms of ``dense_gemm_kernel`` (the exact
fp32 matrix instruction and the split-fp16 one), a checker, and a numpy twin of the split GEMM with the slips it can be told to make.
numpy on the CPU, importable without a GPU.

The GPU suite otherwise feeds these steps ``synth_sae_batch`` and compares whole tensors with ``rel_fro < 1e-4``, every shape with
N % 4 == 0 (the split form only).  tests/test_sae_dense_cases_cpu.py shows which slips of the split form that lets through.

Shapes
------
N 132, d_in 72, d_sae 264 (``BASE``): the smallest that cross every boundary of the 128 x 128 x 32 tile (DG_BM, DG_BN, DG_KSLAB):
  N 132      one full row tile + 4 rows; N % 4 == 0, so the split form; K of G4 / G5 = 4 slabs + 4
  d_in 72    2 slabs + 8 (a K tail inside a slab for G1 / G3); a ragged 72-column tile for G2 / G4 / G5
  d_sae 264  two column tiles + one 8-column chunk.  G2 is split over K in PV_SAE_DENSE_SPLITK = 4: k_chunk = round_up(ceil(264 / 4), 32)
             = 96, so blockIdx.y 0, 1 take [0, 96), [96, 192) (three slabs each), 2 takes [192, 264) (two slabs + 8) and 3 starts at 288 > 264:
             its K range is EMPTY (nk = 0) and it must store a tile of zeros that the finish kernel adds (``splitk_ranges``)
N 134 (``ragged_exact_form``): N % 4 != 0, the kernels take the exact fp32 form on their own.

Normalisation is "none" and b_dec = 0 unless the case says otherwise, so sae_in = x exactly.

The cases (``CASES``)
``exact_grid``        x integers in -3..3, W_enc and b_enc integers / 8, W_dec rows with exactly 16 entries of +-1/4 (row norm exactly 1: the renorm
                      is the identity, asserted on W_dec's bits).  Every scaled operand fits the hi half with lo = 0 and every product and
                      partial sum is exact in fp32, in any order: firing counts, l0, the l1 sum and sae_out must EQUAL the float64 result
                      rounded once (f itself, which dH overwrites, is held through them and through the gates dH != 0).  Behind dY (which
                      carries 2 / (N d)) the general bounds apply.  A pre-activation that is exactly 0 is 0 in both computations.
``ragged_random``     randn operands, both forms (the exact one through the tuning key dense_fp32)
``ragged_exact_form`` the same tensors and two more tokens: N = 134
``outlier``           ``ragged_random`` with x[5, 7] = 2^14 and W_enc[3, 200] = 2^11 (2^14 times the typical magnitude of their tensors: a
                      massive activation): the per-tensor scale puts the lo halves of ordinary entries into the fp16 denormal range, for
                      sae_in and W_enc and, behind them, for f, dY and dH
``no_firing``         b_enc = -2^10, b_dec multiples of 1/4: f == 0, the maxima of f and dH are 0 and their scales clamp.  gW_dec, gW_enc^T,
                      gb_enc exact zeros, sae_out == b_dec, l0 = l1 = 0, nothing NaN or inf
``shrinking``         two steps on ONE engine, x 2^12 and then x: the second must meet its own bounds and equal a fresh engine's step bit for
                      bit (the operand maxima are rebuilt every step)
``tail``              ``ragged_random`` through DG_EPI_ENC_T / DG_EPI_DH_T: activation "tanh-relu", lp_norm 2
``gated_gate_larger`` gated_step (DG_EPI_GENC): x is randn with one switch dimension, 2^19 on tokens [0, 66) and 0 on the others, that W_enc
                      feeds with +-1 into columns [64, 128) and with -1 into columns [0, 64); r_mag = -14 ln 2.  On tokens [0, 66) relu(gate)
                      (out2) reaches 2^19 with magnitudes of 32 behind it -- 2^14 times the token's largest feature_acts (out) -- and holds the
                      maximum of the whole operand; on tokens [66, 132) b_gate opens columns [0, 64), where b_mag lifts feature_acts to
                      2^12 * [14, 15): 2^12 times the token's largest relu(gate), the reverse.  The two planes are ONE operand [2N][F] behind
                      and share one maximum: one that covered feature_acts alone would send relu(gate) past 65504.

Gate condition.  No comparison allows a gate to differ: in the float64 reference every |hidden_pre| (gated: every gate and magnitude
pre-activation) exceeds ``GATE_MARGIN`` = 16 times its own bound in either form.  Tokens that miss it at the seed are nudged (``_settle``)
until the reference alone meets it; tests/test_sae_dense_cases_cpu.py asserts it.

The reference and the bounds
----------------------------
``reference(case)``: float64 of oracle/sae_oracle.py's forward and backward, every quantity with its absolute sum (``<name>_abs`` =
sum_k |a_k| |b_k| per output element).  ``bounds(case, form)``: a bound per element, assembled operation by operation.  u = 2^-24,
gamma(m) = m u / (1 - m u); a GEMM C = A B over K terms whose operands carry the errors dA, dB (A+ = |A| + dA):
  exact form   gamma(K + 4) A+ B+  +  dA B+ + A+ dB
  split form   per operand element, s the tensor's power-of-two scale as ``dg_scale_of`` computes it from the float64 maximum (a tracked
               maximum is that of the stored fp32 tensor: the reference's plus its bound): s a = hi + lo + r with |r| <= max(2^-20 |s a|, 2^-24)
               (two round-toward-zero cuts of 10 bits each; below 2^-14 the fp16 grid is 2^-24), r = 0 for a = 0:  rA B+ + A+ rB + rA rB;
               the dropped lo lo product <= 2^-20 |a| |b|;  the fp32 accumulation of 3 K fp16 products: gamma_23(3 K + 4) (1 + 2^-9) A+ B+
               with u = 2^-23.  The order and the rounding of the matrix instruction's internal adds are not documented; 2^-23 covers
               round-to-nearest and truncation of every add -- this is SUPPOSED, not measured.  Plus dA B+ + A+ dB.
Elementwise steps follow the product and quotient rules (as tests/_sae_backward_cases.py); expf / tanhf / powf are taken to ``ULP_MATH`` = 4
ulp (the HIP device library documents 1-2).  ``SECOND_ORDER`` covers products of errors.  Nothing in a bound is fitted to kernel output.

``check(case, form, got)`` -> (worst error / bound per quantity -- inf for NaN or inf where a number belongs --, messages naming the worst
element by row, column, tile, wave and lane chunk of ``dense_gemm_kernel``'s epilogue).

``twin(case, form, slip=None)``: numpy emulation of the step -- operands scaled, cut into fp16 hi / lo by bit manipulation (round toward
zero, denormal range included, clamped at 65504 as v_cvt_pkrtz does), the three products summed per 32-slab in float64 and rounded to fp32,
epilogues in fp32.  ``SLIPS`` are its wrong versions.
"""
import functools
import math

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
U23 = 2.0 ** -23
SECOND_ORDER = 1.0 + 2.0 ** -10
ULP_MATH = 4.0
GATE_MARGIN = 16.0
DG_BM, DG_BN, DG_KSLAB = 128, 128, 32
PV_SAE_DENSE_SPLITK = 4
DG_AMAX_SLOTS = 256
BASE = (132, 72, 264)
L1 = 3e-3
CASES = ("exact_grid", "ragged_random", "ragged_exact_form", "outlier", "no_firing", "shrinking", "tail", "gated_gate_larger")
FORMS = ("split", "exact")
RELU_QUANTITIES = ("sae_out", "dH", "gW_dec", "gW_enc", "gb_enc", "gb_dec", "loss", "mse", "l1")
GATED_QUANTITIES = ("sae_out", "dP", "dG", "gW_dec", "gW_enc", "gb_gate", "gb_mag", "gr_mag", "gb_dec", "loss", "mse", "l1", "aux")
SLIPS = ("drop_al_bh", "swap_planes_one_kgroup", "flush_lo_denormals", "scale_from_first_slot_only", "stale_max", "out2_not_in_max",
         "k_tail_dropped", "inv_scale_once")


def gamma(m, u=U):
    m = np.asarray(m, F64)
    return m * u / (1.0 - m * u)


def splitk_ranges(K, splits=PV_SAE_DENSE_SPLITK):
    """the K range of every blockIdx.y of G2 (dense_step_body: k_chunk rounded up to the slab)"""
    k_chunk = ((K + splits - 1) // splits + DG_KSLAB - 1) // DG_KSLAB * DG_KSLAB
    return [(min(z * k_chunk, K), min(K, (z + 1) * k_chunk)) if z * k_chunk < K else (z * k_chunk, z * k_chunk) for z in range(splits)]


assert splitk_ranges(264) == [(0, 96), (96, 192), (192, 264), (288, 288)]          # the last split is empty at 264


def _rng(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + (sum(map(ord, k)) if isinstance(k, str) else int(k))) % (2 ** 31)
    return np.random.RandomState(seed)


class Case:
    """kind "relu" / "gated"; P float32 parameters; xs: the inputs of the steps run on one engine (the LAST is the one checked); l1;
    activation / lp_norm; forms: ((form, dense_fp32 tuning value or None), ...) the GPU test runs; renorm: the step's renorm_decoder flag."""

    def __init__(self, name, kind, P, xs, l1=L1, activation="relu", lp_norm=1.0, forms=(("split", None), ("exact", 1)), renorm=False):
        self.name, self.kind, self.P, self.xs, self.l1 = name, kind, P, xs, l1
        self.activation, self.lp_norm, self.forms, self.renorm = activation, lp_norm, forms, renorm
        self.x = xs[-1]
        self.n, self.d_in = self.x.shape
        self.d_sae = P["W_dec"].shape[0]
        for v in list(P.values()) + list(xs):
            v.setflags(write=False)

    def __repr__(self):
        return f"<{self.kind} {self.name} n={self.n} d_in={self.d_in} d_sae={self.d_sae}>"


# ------------------------------------------------------------------------------------------------------------ the cases
def _unit_rows(rs, d_sae, d_in):
    w = rs.standard_normal((d_sae, d_in))
    return (w / np.linalg.norm(w, axis=1, keepdims=True)).astype(F32)


def _random_tensors(n):
    N, D, Fs = BASE
    rs = _rng("ragged")
    x = rs.standard_normal((N + 2, D)).astype(F32)
    P = dict(W_enc=(rs.standard_normal((D, Fs)) / 8.0).astype(F32), W_dec=_unit_rows(rs, Fs, D),
             b_enc=(0.25 * rs.standard_normal(Fs)).astype(F32), b_dec=np.zeros(D, F32))
    return P, x[:n].copy()


def _settle(make, x, frozen=()):
    """nudge tokens until the float64 reference meets the gate condition in both forms: a token with a pre-activation inside the margin
    gets a few 2^-6 of its own size added to one element (never one of ``frozen`` = [(row, col)]); the result depends on the seed alone"""
    rs = _rng("settle", x.shape[0])
    x = x.copy()
    for _ in range(400):
        c = make(x)
        bad = np.zeros(x.shape[0], bool)
        for form in FORMS:
            bad |= gate_margins(c, form)[1]
        if not bad.any():
            return c
        for n in np.flatnonzero(bad):
            while True:
                col = int(rs.randint(x.shape[1]))
                if (int(n), col) not in frozen:
                    break
            scale = 2.0 ** math.floor(math.log2(float(np.median(np.abs(x[n])))))          # (a power of two at the token's own size)
            x[n, col] += F32(2.0 ** -6 * scale) * F32(1 + rs.randint(8))
    raise AssertionError("the gate condition could not be met")


@functools.lru_cache(maxsize=None)
def case(name):
    N, D, Fs = BASE
    if name == "exact_grid":
        rs = _rng("exact_grid")
        x = rs.randint(-3, 4, size=(N, D)).astype(F32)
        W_enc = (rs.randint(-3, 4, size=(D, Fs)) / 8.0).astype(F32)
        b_enc = (rs.randint(-8, 9, size=Fs) / 8.0).astype(F32)
        W_dec = np.zeros((Fs, D), F32)
        for j in range(Fs):
            cols = rs.permutation(D)[:16]
            W_dec[j, cols] = rs.choice([-0.25, 0.25], size=16)
        P = dict(W_enc=W_enc, W_dec=W_dec, b_enc=b_enc, b_dec=np.zeros(D, F32))
        return Case(name, "relu", P, [x], l1=2.0 ** -7, renorm=True)
    if name in ("ragged_random", "ragged_exact_form", "tail", "shrinking"):
        n = N + 2 if name == "ragged_exact_form" else N
        P, x = _random_tensors(N + 2)
        kw = dict(activation="tanh-relu", lp_norm=2.0) if name == "tail" else {}
        if name == "ragged_exact_form":
            kw["forms"] = (("exact", None),)
        # (settled on all 134 tokens: the 132-token cases are its first rows)
        full = _settle(lambda x_: Case(name, "relu", {k: v.copy() for k, v in P.items()}, [x_.copy()], **kw), x)
        xs = [full.x[:n].copy()]
        if name == "shrinking":
            xs = [(xs[0] * F32(4096.0)).astype(F32), xs[0]]
        return Case(name, "relu", {k: v.copy() for k, v in P.items()}, xs, **kw)
    if name == "outlier":
        base = case("ragged_random")
        P = {k: v.copy() for k, v in base.P.items()}
        P["W_enc"][3, 200] = 2.0 ** 11
        x = base.x.copy()
        x[5, 7] = 2.0 ** 14
        return _settle(lambda x_: Case(name, "relu", {k: v.copy() for k, v in P.items()}, [x_.copy()]), x, frozen=((5, 7),))
    if name == "no_firing":
        base = case("ragged_random")
        P = {k: v.copy() for k, v in base.P.items()}
        P["b_enc"] = np.full(Fs, -1024.0, F32)
        P["b_dec"] = (_rng("no_firing").randint(-8, 9, size=D) / 4.0).astype(F32)
        return Case(name, "relu", P, [base.x.copy()])
    if name == "gated_gate_larger":
        # x is randn with one switch dimension: x[n, 0] = 2^19 on tokens [0, 66), 0 on the others.  W_enc[0] is +-1 on columns [64, 128),
        # -1 on columns [0, 64), 0 elsewhere, r_mag = -14 ln 2 everywhere.
        #   tokens [0, 66):   gates of +-2^19 on columns [64, 128) with magnitudes of 32 behind them; columns [0, 64) closed; the rest as below
        #                     without b_mag.  relu(gate) reaches 2^14 times the token's largest feature_acts and holds the operand's maximum.
        #   tokens [66, 132): gates of randn (+ 8 on columns [0, 64), which b_gate opens there), magnitudes of 2^-14 randn + b_mag with b_mag
        #                     in [2^12 * 14, 2^12 * 15) on columns [0, 64): feature_acts reaches 2^12 times the token's largest relu(gate).
        rs = _rng("gated")
        x = rs.standard_normal((N, D)).astype(F32)
        x[:, 0] = 0.0
        x[:N // 2, 0] = 2.0 ** 19
        W_enc = (rs.standard_normal((D, Fs)) / 8.0).astype(F32)
        W_enc[0] = 0.0
        W_enc[0, :64] = -1.0
        W_enc[0, 64:128] = rs.choice([-1.0, 1.0], size=64)
        b_gate = (0.25 * rs.standard_normal(Fs)).astype(F32)
        b_gate[:64] = 8.0
        b_mag = (2.0 ** -16 * rs.standard_normal(Fs)).astype(F32)
        b_mag[:64] = (4096.0 * (14.0 + rs.random_sample(64))).astype(F32)
        P = dict(W_enc=W_enc, W_dec=_unit_rows(rs, Fs, D), b_enc=np.zeros(Fs, F32), b_dec=np.zeros(D, F32), b_gate=b_gate,
                 r_mag=np.full(Fs, -14.0 * math.log(2.0), F32), b_mag=b_mag)
        frozen = tuple((n, 0) for n in range(N))
        return _settle(lambda x_: Case(name, "gated", {k: v.copy() for k, v in P.items()}, [x_.copy()], renorm=True), x, frozen=frozen)
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------------------ float64 reference
def _p64(P):
    return {k: np.asarray(v, F64) for k, v in P.items()}


def reference(c, P=None, step=-1):
    """float64 forward and backward of the case's (last) step; P: other parameters (the decoder rows as the kernels read them after a
    renorm).  ``<q>_abs``: the absolute sums behind q."""
    P = _p64(c.P if P is None else P)
    x = np.asarray(c.xs[step], F64)
    N, D = x.shape
    We, Wd, bd = P["W_enc"], P["W_dec"], P["b_dec"]
    aWe, aWd = np.abs(We), np.abs(Wd)
    r = dict(x=x, P=P, n=N)
    si = x - bd
    asi = np.abs(si)
    bm = x.mean(axis=0, keepdims=True)
    cx = x - bm
    nf = np.sqrt((cx ** 2).sum(axis=1, keepdims=True))
    gs = 2.0 / (N * D)
    r.update(sae_in=si, bm=bm, nf=nf, gs=gs)
    if c.kind == "relu":
        hp0 = si @ We
        hp = hp0 + P["b_enc"]
        f = np.maximum(hp, 0.0)
        if c.activation == "tanh-relu":
            f = np.tanh(f)
        fire = hp > 0
        pre, pre_abs = f @ Wd, f @ aWd
        out = pre + bd
        e = out - x
        dY = gs * e / nf
        t = e ** 2 / nf
        mse = t.sum() / (N * D)
        p = float(c.lp_norm)
        if p == 1.0:
            S = tok = lpt = None
            l1 = c.l1 * f.sum() / N
            g = dY @ Wd.T + c.l1 / N
        else:
            S = (f ** p).sum(axis=1, keepdims=True)
            tok = S ** (1.0 / p)
            with np.errstate(divide="ignore"):
                lpt = np.where(S > 0, c.l1 / N * S ** (1.0 / p - 1.0), 0.0)
            l1 = c.l1 * tok.sum() / N
            g = dY @ Wd.T + lpt * np.where(fire, f ** (p - 1.0), 0.0)
        dF = dY @ Wd.T
        if c.activation == "tanh-relu":
            g = g * (1.0 - f * f)
        dH = np.where(fire, g, 0.0)
        gbe = dH.sum(axis=0)
        r.update(hp0=hp0, hp0_abs=asi @ aWe, hidden_pre=hp, f=f, fire=fire, pre=pre, pre_abs=pre_abs, sae_out=out, e=e, dY=dY, t=t, mse=mse,
                 l1=l1, loss=mse + l1, lp_S=S, lp_tokn=tok, lp_tok=lpt, dF=dF, dF_abs=np.abs(dY) @ aWd.T, g=g, dH=dH, gb_enc=gbe,
                 gb_enc_abs=np.abs(dH).sum(axis=0), gW_dec=f.T @ dY, gW_dec_abs=f.T @ np.abs(dY), gW_enc=dH.T @ si,
                 gW_enc_abs=np.abs(dH).T @ asi, gb_dec=dY.sum(axis=0) - We @ gbe, counts=fire.sum(axis=0), l0=fire.sum() / N)
        return r
    # gated
    p0 = si @ We
    er = np.exp(P["r_mag"])
    gp = p0 + P["b_gate"]
    mp = p0 * er + P["b_mag"]
    active = gp > 0
    pg = np.maximum(gp, 0.0)
    f = np.where(active, np.maximum(mp, 0.0), 0.0)
    on_f = active & (mp > 0)
    out = f @ Wd + bd
    via = pg @ Wd + bd
    e = out - x
    e2 = via - si
    dY = gs * e / nf
    dVia = 2.0 / N * e2
    t = e ** 2 / nf
    mse = t.sum() / (N * D)
    wn = np.linalg.norm(Wd, axis=1)
    add = c.l1 / N
    l1 = c.l1 * (pg * wn).sum() / N
    aux = (e2 ** 2).sum() / N
    dM0, dG0 = dY @ Wd.T, dVia @ Wd.T
    dM = np.where(on_f, dM0, 0.0)
    dG = np.where(active, dG0 + add * wn, 0.0)
    dP = dM * er + dG
    gbm, gbg = dM.sum(axis=0), dG.sum(axis=0)
    sdmf = (dM * f).sum(axis=0)
    pgsum = pg.sum(axis=0)
    l1rows = add * pgsum[:, None] * (Wd / wn[:, None])
    dps = er * gbm + gbg
    r.update(p0=p0, p0_abs=asi @ aWe, er=er, gate_pre=gp, mag_pre=mp, active=active, on_f=on_f, pg=pg, f=f, sae_out=out, via=via, e=e, e2=e2,
             dY=dY, dVia=dVia, t=t, mse=mse, wn=wn, l1=l1, aux=aux, loss=mse + l1 + aux, dM0=dM0, dG0=dG0, dM=dM, dG=dG, dP=dP, gb_mag=gbm,
             gb_gate=gbg, sdmf=sdmf, gr_mag=sdmf - P["b_mag"] * gbm, pgsum=pgsum, l1rows=l1rows,
             gW_dec=f.T @ dY + pg.T @ dVia + l1rows, gW_dec_abs=f.T @ np.abs(dY) + pg.T @ np.abs(dVia),
             gW_enc=dP.T @ si, gW_enc_abs=np.abs(dP).T @ asi, dpsum=dps,
             gb_dec=dY.sum(axis=0) + 2.0 * dVia.sum(axis=0) - We @ dps, counts=on_f.sum(axis=0), l0=on_f.sum() / N,
             pre_abs=f @ aWd, via_abs=pg @ aWd)
    return r


# ------------------------------------------------------------------------------------------------------------ the bounds
def scale_of(maxabs):
    """dg_scale_of: the exponent field of the fp32 maximum clamped to [24, 250] -> (s, 1 / s); the largest entry lands in [2^13, 2^14)"""
    bits = int(np.asarray(maxabs, F32).view(np.uint32))
    e = min(max((bits >> 23) & 0xFF, 24), 250)
    return 2.0 ** (140 - e), 2.0 ** (e - 140)


def _up32(v):
    """a float64 maximum as the smallest fp32 not below it"""
    f = F32(v)
    return f if F64(f) >= v else np.nextafter(f, F32(np.inf))


def _gemm_bound(Aabs, Aerr, Babs, Berr, form):
    """bound of A @ B, A [M, K], B [K, N] (module docstring)"""
    K = Aabs.shape[1]
    Au, Bu = Aabs + Aerr, Babs + Berr
    AB = Au @ Bu
    prop = Aerr @ Bu + Au @ Berr
    if form == "exact":
        return gamma(K + 4) * AB + prop
    sa, sb = scale_of(_up32(Au.max()))[0], scale_of(_up32(Bu.max()))[0]
    rA = np.where(Au > 0, np.maximum(2.0 ** -20 * Au, 2.0 ** -24 / sa), 0.0)
    rB = np.where(Bu > 0, np.maximum(2.0 ** -20 * Bu, 2.0 ** -24 / sb), 0.0)
    return (gamma(3 * K + 4, U23) * (1.0 + 2.0 ** -9) + 2.0 ** -20) * AB + rA @ Bu + Au @ rB + rA @ rB + prop


def _loss_norm(r):
    """(nf_err, rel_nf): the loss normaliser ||x_n - batch mean|| as tests/_sae_backward_cases.py bounds it"""
    x, N, D = r["x"], r["n"], r["x"].shape[1]
    bm_err = gamma(N + 2) * np.abs(x).mean(axis=0, keepdims=True)
    cx = x - r["bm"]
    c_err = bm_err + U * np.abs(cx)
    cn = r["nf"] ** 2
    cn_err = gamma(D + 1) * cn + (2 * np.abs(cx) * c_err + c_err ** 2).sum(axis=1, keepdims=True)
    nf_err = cn_err / r["nf"] + 2 * U * r["nf"]
    return nf_err, nf_err / (r["nf"] - nf_err)


def bounds(c, form, P=None, step=-1, ref=None):
    """-> {quantity: bound per element} for the case's (last) step in the given form, beside the reference it was built from (``ref``)"""
    assert form in FORMS, form
    r = reference(c, P, step) if ref is None else ref
    P, x, N = r["P"], r["x"], r["n"]
    D = x.shape[1]
    Fs = P["W_dec"].shape[0]
    We, Wd, bd = P["W_enc"], P["W_dec"], P["b_dec"]
    aWe, aWd = np.abs(We), np.abs(Wd)
    si, asi = r["sae_in"], np.abs(r["sae_in"])
    si_err = U * asi if np.any(bd != 0) else np.zeros_like(si)
    z_in, z_w = np.zeros_like(si), np.zeros_like(Wd)
    nf, gs = r["nf"], r["gs"]
    nf_err, rel_nf = _loss_norm(r)
    S = PV_SAE_DENSE_SPLITK
    b = dict(ref=r, sae_in=si_err)

    def finish(pre_b, out, e):
        out_err = pre_b + U * np.abs(out)
        e_err = out_err + U * np.abs(e)
        dY = gs * e / nf
        dY_err = gs / nf * e_err * (1 + rel_nf) + np.abs(dY) * (rel_nf + 6 * U)
        t = r["t"]
        t_err = (2 * np.abs(e) * e_err + e_err ** 2) / nf * (1 + rel_nf) + t * rel_nf
        mse_b = (t_err.sum() + gamma(N + D + 8) * t.sum()) / (N * D) + 4 * U * r["mse"]
        return out_err, dY_err, mse_b

    if c.kind == "relu":
        f, fire = r["f"], r["fire"]
        hp_b = _gemm_bound(asi, si_err, aWe, z_w.T, form) + U * (np.abs(r["hp0"]) + np.abs(r["hidden_pre"]))
        f_err = np.where(fire, hp_b, 0.0)
        if c.activation == "tanh-relu":
            f_err = np.where(fire, hp_b + ULP_MATH * U * f, 0.0)               # |d tanh| <= 1
        pre_b = _gemm_bound(f, f_err, aWd, z_w, form) + gamma(S + 2) * (r["pre_abs"] + np.abs(bd))
        out_err, dY_err, mse_b = finish(pre_b, r["sae_out"], r["e"])
        adY = np.abs(r["dY"])
        dF_b = _gemm_bound(adY, dY_err, aWd.T, z_w.T, form)
        p = float(c.lp_norm)
        if p == 1.0:
            add = c.l1 / N
            g1, g1_err = r["dF"] + add, dF_b + U * (np.abs(r["dF"]) + add + np.abs(r["dF"] + add))
            l1_b = gamma(N * Fs + 8) * r["l1"] + c.l1 * f_err.sum() / N + 4 * U * r["l1"]
        else:
            Sp = r["lp_S"]
            with np.errstate(divide="ignore", invalid="ignore"):
                fp1 = np.where(fire, f ** (p - 1.0), 0.0)
                fp2 = np.where(fire, f ** (p - 2.0), 0.0)
                S_err = gamma(Fs + 8) * Sp + (p * fp1 * f_err + ULP_MATH * U * fp1 * f).sum(axis=1, keepdims=True)
                relS = np.where(Sp > 0, S_err / np.maximum(Sp - S_err, 1e-300), 0.0)
            tok_err = r["lp_tokn"] * (relS / p + (ULP_MATH + 2) * U)
            lpt = r["lp_tok"]
            lpt_err = lpt * (abs(1.0 / p - 1.0) * relS + (ULP_MATH + 4) * U)
            term = lpt * fp1
            term_err = lpt_err * fp1 + lpt * ((p - 1.0) * fp2 * f_err + ULP_MATH * U * fp1) + U * term
            g1 = r["dF"] + term
            g1_err = dF_b + term_err + U * (np.abs(r["dF"]) + np.abs(term) + np.abs(g1))
            l1_b = c.l1 * tok_err.sum() / N + gamma(N + 8) * r["l1"] + 4 * U * r["l1"]
        if c.activation == "tanh-relu":
            om = 1.0 - f * f
            g_err = g1_err * om + np.abs(g1) * (2 * f * f_err + 3 * U) + U * np.abs(g1 * om)
        else:
            g_err = g1_err
        dH_err = np.where(fire, g_err, 0.0)
        adH = np.abs(r["dH"])
        gbe_b = gamma(N + 8) * r["gb_enc_abs"] + dH_err.sum(axis=0)
        b.update(hidden_pre=hp_b, f=f_err + U * f, sae_out=out_err, dY=dY_err, dH=dH_err, mse=mse_b, l1=l1_b,
                 loss=mse_b + l1_b + 2 * U * r["loss"],
                 gW_dec=_gemm_bound(f.T, f_err.T, adY, dY_err, form), gW_enc=_gemm_bound(adH.T, dH_err.T, asi, si_err, form), gb_enc=gbe_b,
                 gb_dec=gamma(N + Fs + 4) * (adY.sum(axis=0) + aWe @ np.abs(r["gb_enc"])) + dY_err.sum(axis=0) + aWe @ gbe_b)
        quantities = RELU_QUANTITIES + ("f", "hidden_pre", "dY")
    else:
        er = r["er"]
        er_err = ULP_MATH * U * er
        p0_b = _gemm_bound(asi, si_err, aWe, z_w.T, form)
        gp_b = p0_b + U * (np.abs(r["p0"]) + np.abs(r["gate_pre"]))
        mp_b = p0_b * er + np.abs(r["p0"]) * er_err + U * (np.abs(r["p0"] * er) + np.abs(r["mag_pre"]))
        active, on_f, f, pg = r["active"], r["on_f"], r["f"], r["pg"]
        f_err, pg_err = np.where(on_f, mp_b, 0.0), np.where(active, gp_b, 0.0)
        hs, hs_err = np.concatenate([f, pg]), np.concatenate([f_err, pg_err])             # ONE operand [2N][F]: one maximum
        pre2_b = _gemm_bound(hs, hs_err, aWd, z_w, form)
        pre_b = pre2_b[:N] + gamma(S + 2) * (r["pre_abs"] + np.abs(bd))
        out_err, dY_err, mse_b = finish(pre_b, r["sae_out"], r["e"])
        e2 = r["e2"]
        e2_err = pre2_b[N:] + gamma(S + 3) * (r["via_abs"] + np.abs(bd) + asi) + si_err
        dVia_err = 2.0 / N * e2_err + 2 * U * np.abs(r["dVia"])
        aux_b = (2 * np.abs(e2) * e2_err + e2_err ** 2).sum() / N + gamma(N + D + 8) * r["aux"]
        dYs, dYs_err = np.abs(np.concatenate([r["dY"], r["dVia"]])), np.concatenate([dY_err, dVia_err])
        wn_dev = np.abs(r["wn"] - 1.0) + gamma(D + 4)                           # the kernels take the renormed rows as unit rows
        add = c.l1 / N
        pgsum_b = gamma(N + 8) * r["pgsum"] + pg_err.sum(axis=0)
        l1rows_b = add * pgsum_b[:, None] * aWd / r["wn"][:, None] + np.abs(r["l1rows"]) * gamma(D + 8)
        gWd_b = _gemm_bound(hs.T, hs_err.T, dYs, dYs_err, form)
        gWd_b = gWd_b + l1rows_b + U * (np.abs(r["gW_dec"]) + np.abs(r["l1rows"]))
        d2_b = _gemm_bound(dYs, dYs_err, aWd.T, z_w.T, form)                  # (rows [0, N) and [N, 2N) are two launches on the SAME maxima)
        dM_err = np.where(on_f, d2_b[:N], 0.0)
        dG_err = np.where(active, d2_b[N:] + U * (np.abs(r["dG0"]) + add + np.abs(r["dG0"] + add)) + add * wn_dev, 0.0)
        adM, adG = np.abs(r["dM"]), np.abs(r["dG"])
        dP_err = dM_err * er + adM * er_err + dG_err + U * (adM * er + np.abs(r["dP"]))
        gbm_b = gamma(N + 8) * adM.sum(axis=0) + dM_err.sum(axis=0)
        gbg_b = gamma(N + 8) * adG.sum(axis=0) + dG_err.sum(axis=0)
        sdmf_b = gamma(N + 9) * (adM * f).sum(axis=0) + (dM_err * f + adM * f_err).sum(axis=0)
        abm = np.abs(P["b_mag"])
        grm_b = sdmf_b + abm * gbm_b + U * (np.abs(r["sdmf"]) + 2 * abm * np.abs(r["gb_mag"]) + np.abs(r["gr_mag"]))
        dps_b = er * gbm_b + er_err * np.abs(r["gb_mag"]) + gbg_b + U * (2 * er * np.abs(r["gb_mag"]) + np.abs(r["gb_gate"]) + np.abs(r["dpsum"]))
        adY, adV = np.abs(r["dY"]), np.abs(r["dVia"])
        l1_b = gamma(N * Fs + 8) * r["l1"] + c.l1 * pg_err.sum() / N + r["l1"] * wn_dev.max() + 4 * U * r["l1"]
        b.update(gate_pre=gp_b, mag_pre=mp_b, sae_out=out_err, dY=dY_err, dVia=dVia_err, dP=dP_err, dG=dG_err, mse=mse_b, l1=l1_b,
                 aux=aux_b + 4 * U * r["aux"], loss=mse_b + l1_b + aux_b + 4 * U * r["loss"], gW_dec=gWd_b,
                 gW_enc=_gemm_bound(np.abs(r["dP"]).T, dP_err.T, asi, si_err, form), gb_mag=gbm_b, gb_gate=gbg_b, gr_mag=grm_b,
                 gb_dec=gamma(N + Fs + 8) * (adY.sum(axis=0) + 2 * adV.sum(axis=0) + aWe @ np.abs(r["dpsum"])) + dY_err.sum(axis=0)
                 + 2 * dVia_err.sum(axis=0) + aWe @ dps_b)
        quantities = GATED_QUANTITIES + ("gate_pre", "mag_pre", "dY", "dVia")
    for q in quantities:
        b[q] = b[q] * SECOND_ORDER
    return b


def gate_margins(c, form, P=None):
    """-> (the smallest |pre-activation| / its bound over the step, tokens that miss GATE_MARGIN).  An exact zero of ``exact_grid`` is
    exempt: there every product and partial sum is exact, so it is a zero in the kernel too."""
    b = bounds(c, form, P)
    r = b["ref"]
    worst, bad = math.inf, np.zeros(r["n"], bool)
    for q in (("hidden_pre",) if c.kind == "relu" else ("gate_pre", "mag_pre")):
        v = np.abs(r[q])
        ratio = v / b[q]
        if c.name == "exact_grid":
            ratio = np.where(v == 0, np.inf, ratio)
        worst = min(worst, float(ratio.min()))
        bad |= (ratio <= GATE_MARGIN).any(axis=1)
    return worst, bad


# ------------------------------------------------------------------------------------------------------------ the checker
def _ratios(got, ref, bound):
    got = np.asarray(got, F64)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return np.where(np.isfinite(got), r, np.inf)


def epilogue_place(row, col):
    """where dense_gemm_kernel's epilogue handles element (row, col) of its output"""
    rm, cn = row % DG_BM, col % DG_BN
    return (f"tile ({row // DG_BM}, {col // DG_BN}) wave {(rm // 64) * 2 + cn // 64} lane {((rm % 64) % 8) * 8 + (cn % 64) // 8} "
            f"(pass {(rm % 64) // 8}, chunk {(cn % 64) // 8}, element {cn % 8})")


def check(c, form, got, P=None, bnd=None):
    """got: whatever of the case's quantities the caller has (gradients in the kernels' layouts: gW_enc transposed [d_sae, d_in]); also
    f / hidden gates (``gates`` [N, d_sae] bool), fire_count, l0, and for ``shrinking`` ``fresh``: the same dict from a fresh engine, to be
    equal bit for bit.  -> (ratios, messages)"""
    b = bounds(c, form, P) if bnd is None else bnd
    r = b["ref"]
    ratios, msgs = {}, []

    def exact(name, ok, what):
        ratios[name] = 0.0 if ok else math.inf
        if not ok:
            msgs.append(f"{name}: {what() if callable(what) else what}")

    names = RELU_QUANTITIES + ("f",) if c.kind == "relu" else GATED_QUANTITIES
    for q in names:
        if q not in got:
            continue
        g = np.asarray(got[q], F64)
        if g.shape != np.shape(r[q]):
            exact(q, False, f"shape {g.shape}, expected {np.shape(r[q])}")
            continue
        rt = _ratios(g, r[q], b[q])
        worst = float(rt.max())
        ratios[q] = worst
        if not worst <= 1.0:
            if g.ndim == 2:
                w = tuple(int(i) for i in np.unravel_index(int(np.argmax(rt)), rt.shape))
                where = f"row {w[0]} column {w[1]}" + (f", {epilogue_place(*w)}" if q != "sae_out" else "")
                msgs.append(f"{q}: {where}: got {g[w]!r}, float64 {r[q][w]!r}, bound {b[q][w]:.3e}, ratio {worst:.3g}")
            elif g.ndim == 1:
                w = int(np.argmax(rt))
                msgs.append(f"{q}: element {w}: got {g[w]!r}, float64 {r[q][w]!r}, bound {b[q][w]:.3e}, ratio {worst:.3g}")
            else:
                msgs.append(f"{q}: got {float(g)!r}, float64 {float(r[q])!r}, bound {float(b[q]):.3e}, ratio {worst:.3g}")
    want_gates = r["fire"] if c.kind == "relu" else r["on_f"]
    if "gates" in got:
        bad = np.argwhere(np.asarray(got["gates"], bool) != want_gates)
        exact("gates", bad.size == 0, lambda: f"{len(bad)} gates differ from float64, first at row {bad[0][0]} column {bad[0][1]}, "
              f"{epilogue_place(int(bad[0][0]), int(bad[0][1]))}")
    if "fire_count" in got:
        j = np.flatnonzero(np.asarray(got["fire_count"], F64) != r["counts"])
        exact("fire_count", j.size == 0, lambda: f"feature {j[0]}: {got['fire_count'][j[0]]} counted, {r['counts'][j[0]]} fire")
    if "l0" in got:
        want = F32(r["counts"].sum()) * (F32(1.0) / F32(r["n"]))               # reduce_sum_kernel: the exact count times fp32(1 / N)
        exact("l0", F32(got["l0"]) == want, f"scalars[2] = {got['l0']!r}, expected {want!r}")
    if c.name == "exact_grid":
        if "sae_out" in got:
            bad = np.argwhere(np.asarray(got["sae_out"], F32) != r["sae_out"].astype(F32))
            exact("sae_out_exact", bad.size == 0, lambda: f"{len(bad)} elements differ from float64 rounded once, first at {bad[0].tolist()}")
        if "f" in got:
            bad = np.argwhere(np.asarray(got["f"], F32) != r["f"].astype(F32))
            exact("f_exact", bad.size == 0, lambda: f"{len(bad)} elements differ, first at {bad[0].tolist()}, {epilogue_place(*bad[0].tolist())}")
        if "l1" in got:
            want = F32(r["f"].sum()) * (F32(c.l1) / F32(r["n"]))               # the exact sum of f times fp32(l1 / N)
            exact("l1_exact", F32(got["l1"]) == want, f"scalars[4] = {got['l1']!r}, expected {want!r}")
    if c.name == "no_firing":
        for q in ("gW_dec", "gW_enc", "gb_enc"):
            if q in got:
                exact(q + "_zero", bool((np.asarray(got[q]) == 0).all()), "not exactly zero")
        if "sae_out" in got:
            exact("sae_out_is_b_dec", bool((np.asarray(got["sae_out"], F32) == np.asarray(r["P"]["b_dec"], F32)[None, :]).all()), "sae_out != b_dec")
        for q in ("l0", "l1"):
            if q in got:
                exact(q + "_zero", float(got[q]) == 0.0, f"{q} = {got[q]!r}")
    if "fresh" in got:
        for q, v in got["fresh"].items():
            if q in got and not isinstance(v, dict):
                a, f_ = np.ascontiguousarray(np.asarray(got[q], F32)), np.ascontiguousarray(np.asarray(v, F32))
                exact(q + "_fresh_bits", a.shape == f_.shape and np.array_equal(a.view(np.uint32), f_.view(np.uint32)),
                      "differs from a fresh engine's step on the same input")
    return ratios, msgs


def passes(ratios):
    return all(v <= 1.0 for v in ratios.values())


def fmt(ratios):
    return " ".join(f"{k_}={v:.3g}" for k_, v in ratios.items())


# ------------------------------------------------------------------------------------------------------------ the twin
def rtz16(v):
    """float32 -> the fp16 value toward zero, as float32 (v_cvt_pkrtz_f16_f32): the low 13 mantissa bits dropped, more below 2^-14 where the
    fp16 grid is 2^-24, zero below 2^-24, 65504 above"""
    b = np.ascontiguousarray(v, F32).view(np.uint32)
    sign, mag = b & np.uint32(0x80000000), b & np.uint32(0x7FFFFFFF)
    e = (mag >> np.uint32(23)).astype(np.int64) - 127
    drop = (13 + np.clip(-14 - e, 0, 10)).astype(np.uint32)
    m = mag & ~((np.uint32(1) << drop) - np.uint32(1))
    m = np.where(e < -24, np.uint32(0), m)
    m = np.minimum(m, np.uint32(0x477FE000))
    return (m | sign).astype(np.uint32).view(F32)


def split16(a, s):
    """(hi, lo) of dg_split4 for the float32 tensor a and the scale s"""
    sx = (np.asarray(a, F32) * F32(s)).astype(F32)
    hi = rtz16(sx)
    return hi, rtz16((sx - hi).astype(F32))


def _max32(t, producer, slip):
    """the tracked maximum of a tensor: all 256 slots, or with ``scale_from_first_slot_only`` slot 0 -- the first 64 threads of
    dense_absmax3_kernel (256 floats), block 0 wave 0 of an epilogue (a 64 x 64 block), token 0 of the finish kernel"""
    t = np.abs(np.asarray(t, F32))
    if slip == "scale_from_first_slot_only":
        t = {"absmax3": t.ravel()[:256], "epilogue": t[:64, :64], "finish": t[:1]}[producer]
    return F32(t.max()) if t.size else F32(0)


def tgemm(A, B, form, ma, mb, slip=None, ranges=None):
    """A [M, K] @ B [K, N] as dense_gemm_kernel computes it, one result per K range ([splits, M, N] float32).  ma, mb: the tracked maxima."""
    A, B = np.asarray(A, F32), np.asarray(B, F32)
    K = A.shape[1]
    ranges = [(0, K)] if ranges is None else ranges
    out = np.zeros((len(ranges), A.shape[0], B.shape[1]), F32)
    if form == "split":
        (sa, ia), (sb, ib) = scale_of(ma), scale_of(mb)
        ah, al = (v.astype(F64) for v in split16(A, sa))
        bh, bl = (v.astype(F64) for v in split16(B, sb))
        if slip == "flush_lo_denormals":
            al, bl = np.where(np.abs(al) < 2.0 ** -14, 0.0, al), np.where(np.abs(bl) < 2.0 ** -14, 0.0, bl)
    for z, (k0, k1) in enumerate(ranges):
        acc = np.zeros(out.shape[1:], F32)
        for kb in range(k0, k1, DG_KSLAB):
            ke = min(kb + DG_KSLAB, k1)
            if slip == "k_tail_dropped" and ke - kb < DG_KSLAB:
                continue
            sl = slice(kb, ke)
            if form == "exact":
                part = A[:, sl].astype(F64) @ B[sl].astype(F64)
            else:
                h, l = ah[:, sl], al[:, sl]
                if slip == "swap_planes_one_kgroup" and ke - kb > 8:         # k-group 1 (k = 8..15 of the slab) of A: the planes swapped
                    h, l = h.copy(), l.copy()
                    h[:, 8:16], l[:, 8:16] = al[:, sl][:, 8:16], ah[:, sl][:, 8:16]
                part = h @ bl[sl] + h @ bh[sl]
                if slip != "drop_al_bh":
                    part = part + l @ bh[sl]
            acc = (acc.astype(F64) + part).astype(F32)
        if form == "split":
            acc = (acc * F32(ia)).astype(F32)
            if slip != "inv_scale_once":
                acc = (acc * F32(ib)).astype(F32)
        out[z] = acc
    return out


def twin(c, form, slip=None, P=None, fresh=False):
    """The case's steps in float32 as the kernels are structured (the LAST step's results): prep, the five GEMMs through ``tgemm``, the
    epilogues and small kernels in fp32.  ``stale_max``: the maxima of a step start from the step before instead of zero.  fresh: only the
    last input, as a fresh engine would see it."""
    assert form in FORMS and (slip is None or slip in SLIPS), (form, slip)
    P = {k: np.asarray(v, F32) for k, v in (c.P if P is None else P).items()}
    got, carried = None, {}
    for x in (c.xs[-1:] if fresh else c.xs):
        got, maxima = _twin_step(c, form, slip, P, np.asarray(x, F32), carried if slip == "stale_max" else {})
        carried = maxima
    return got


def _twin_step(c, form, slip, P, x, stale):
    f32 = F32
    N, D = x.shape
    We, Wd, bd = P["W_enc"], P["W_dec"], P["b_dec"]
    Fs = Wd.shape[0]
    maxima = {}

    def mx(name, t, producer):
        m = max(_max32(t, producer, slip), stale.get(name, f32(0)))
        maxima[name] = m
        return m

    si = (x - bd).astype(f32)
    bm = (x.sum(axis=0, keepdims=True, dtype=f32) * (f32(1) / f32(N))).astype(f32)
    nf = np.sqrt(((x - bm) ** 2).sum(axis=1, keepdims=True, dtype=f32)).astype(f32)
    m_x, m_we, m_wd = mx("x", si, "absmax3"), mx("W_enc", We.T, "absmax3"), mx("W_dec", Wd, "absmax3")
    gs = f32(2.0) / (f32(N) * f32(D))
    ranges = splitk_ranges(Fs)

    def finish(kp, out_rows):
        a = kp[0]
        for z in range(1, kp.shape[0]):
            a = (a + kp[z]).astype(f32)
        return (a[out_rows] + bd).astype(f32)

    if c.kind == "relu":
        p0 = tgemm(si, We, form, m_x, m_we, slip)[0]
        f = np.maximum((p0 + P["b_enc"]).astype(f32), f32(0))
        if c.activation == "tanh-relu":
            f = np.tanh(f.astype(F64)).astype(f32)
        fire = f > 0
        m_f = mx("f", f, "epilogue")
        o = finish(tgemm(f, Wd, form, m_f, m_wd, slip, ranges), slice(None))
        e = (o - x).astype(f32)
        dY = (gs * e / nf).astype(f32)
        mse = f32(((e * e) / nf).sum(dtype=f32) * (f32(1) / (f32(N) * f32(D))))
        m_dy = mx("dY", dY, "finish")
        p = float(c.lp_norm)
        v = tgemm(dY, Wd.T, form, m_dy, m_wd, slip)[0]
        if p == 1.0:
            l1 = f32(f.sum(dtype=f32) * (f32(c.l1) / f32(N)))
            g = (v + f32(c.l1) / f32(N)).astype(f32)
        else:
            Sp = np.where(fire, f.astype(F64) ** p, 0.0).astype(f32).sum(axis=1, keepdims=True, dtype=f32)
            tok = np.where(Sp > 0, Sp.astype(F64) ** (1.0 / p), 0.0).astype(f32)
            lpt = np.where(Sp > 0, F64(f32(c.l1) / f32(N)) * Sp.astype(F64) ** (1.0 / p - 1.0), 0.0).astype(f32)
            l1 = f32(tok.sum(dtype=f32) * (f32(c.l1) / f32(N)))
            g = (v + (lpt * np.where(fire, f.astype(F64) ** (p - 1.0), 0.0).astype(f32)).astype(f32)).astype(f32)
        if c.activation == "tanh-relu":
            g = (g * (f32(1) - f * f).astype(f32)).astype(f32)
        dH = np.where(fire, g, f32(0)).astype(f32)
        m_dh = mx("dH", dH, "epilogue")
        gbe = dH.sum(axis=0, dtype=f32)
        got = dict(f=f, gates=fire, sae_out=o, dY=dY, dH=dH, mse=mse, l1=l1, loss=f32(mse + l1), l0=f32(fire.sum()) * (f32(1) / f32(N)),
                   fire_count=fire.sum(axis=0).astype(f32), gW_dec=tgemm(f.T, dY, form, m_f, m_dy, slip)[0],
                   gW_enc=tgemm(dH.T, si, form, m_dh, m_x, slip)[0], gb_enc=gbe,
                   gb_dec=(dY.sum(axis=0, dtype=f32) - (We * gbe[None, :]).sum(axis=1, dtype=f32)).astype(f32))
        return got, maxima
    er = np.exp(P["r_mag"].astype(F64)).astype(f32)
    p0 = tgemm(si, We, form, m_x, m_we, slip)[0]
    gp = (p0 + P["b_gate"]).astype(f32)
    mp = ((p0 * er).astype(f32) + P["b_mag"]).astype(f32)
    active = gp > 0
    pg = np.maximum(gp, f32(0))
    f = np.where(active, np.maximum(mp, f32(0)), f32(0)).astype(f32)
    on_f = f > 0
    hs = np.concatenate([f, pg])
    m_hs = mx("hs", f if slip == "out2_not_in_max" else hs, "epilogue")
    kp = tgemm(hs, Wd, form, m_hs, m_wd, slip, ranges)
    o = finish(kp, slice(0, N))
    e = (o - x).astype(f32)
    e2 = (finish(kp, slice(N, 2 * N)) - si).astype(f32)
    dY = (gs * e / nf).astype(f32)
    dVia = ((f32(2) / f32(N)) * e2).astype(f32)
    mse = f32(((e * e) / nf).sum(dtype=f32) * (f32(1) / (f32(N) * f32(D))))
    aux = f32((e2 * e2).sum(dtype=f32) * (f32(1) / f32(N)))
    l1 = f32(pg.sum(dtype=f32) * (f32(c.l1) / f32(N)))
    dYs = np.concatenate([dY, dVia])
    m_dy = mx("dYs", dYs, "finish")
    add = f32(c.l1) / f32(N)
    gWd = tgemm(hs.T, dYs, form, m_hs, m_dy, slip)[0]
    dM = np.where(on_f, tgemm(dY, Wd.T, form, m_dy, m_wd, slip)[0], f32(0)).astype(f32)
    dG = np.where(active, (tgemm(dVia, Wd.T, form, m_dy, m_wd, slip)[0] + add).astype(f32), f32(0)).astype(f32)
    dP = ((dM * er).astype(f32) + dG).astype(f32)
    m_dp = mx("dP", dP, "epilogue")
    gbm, gbg = dM.sum(axis=0, dtype=f32), dG.sum(axis=0, dtype=f32)
    sdmf = (dM * f).astype(f32).sum(axis=0, dtype=f32)
    wn = np.sqrt((Wd * Wd).sum(axis=1, dtype=f32)).astype(f32)
    gWd = (gWd + ((add * pg.sum(axis=0, dtype=f32) / wn)[:, None] * Wd).astype(f32)).astype(f32)
    dps = ((er * gbm).astype(f32) + gbg).astype(f32)
    gbd = (dY.sum(axis=0, dtype=f32) - (We * dps[None, :]).sum(axis=1, dtype=f32)).astype(f32)
    gbd = (gbd + f32(2) * dVia.sum(axis=0, dtype=f32)).astype(f32)
    got = dict(gates=on_f, sae_out=o, dY=dY, dVia=dVia, dP=dP, dG=dG, mse=mse, l1=l1, aux=aux, loss=f32(f32(mse + l1) + aux),
               l0=f32(on_f.sum()) * (f32(1) / f32(N)), fire_count=on_f.sum(axis=0).astype(f32), gW_dec=gWd,
               gW_enc=tgemm(dP.T, si, form, m_dp, m_x, slip)[0], gb_mag=gbm, gb_gate=gbg,
               gr_mag=(sdmf - (P["b_mag"] * gbm).astype(f32)).astype(f32), gb_dec=gbd)
    return got, maxima
