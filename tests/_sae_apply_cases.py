"""Planted states for the SAE optimizer step (``pv_sae_apply``: clip -> remove the gradient parallel to the decoder rows -> Adam, and the
shadows of the encoder it keeps in step), a float64 reference, per-element bounds, a checker, and a float32 twin of the kernels' structure
with the slips it can be told to make.  numpy on the CPU, importable without a GPU.

The GPU suite otherwise compares parameters and moments after one or two steps at lr = 1e-3 from zero moments with ``rel_fro < 1e-4``: one
step moves a weight by at most lr, so the whole update hides under the weight's own norm, and nothing reads W_enc16T, enc_colsq or
dec_inv_norm (tests/test_sae_apply_cases_cpu.py shows which slips that lets through).

The cases (``make``)
--------------------
d_sae = 72 (two whole 32-feature tiles of ``wenc_rows_kernel`` + 8 rows; 18 four-row workgroups of the row kernels), d_in from ``WIDTHS``.
Feature row j is of class ``ROW_CLASSES[j % 8]``, so every class sits in a full tile and in the ragged last one:
  zero                 g = m = v = 0: the row must keep its bits (m' = 0, v' = 0, the quotient 0 / eps = 0)
  zero_g_live_moments  g = 0, planted m, v: the moments still decay and the weight still moves
  first_step           m = v = 0, |g| = 2^e, e uniform in [-20, 10]
  eps_regime           sqrt(v' / bc2) within 2^+-2.5 of eps = 1e-8 (half of v' from v, half from the clipped g): eps decides the quotient
  parallel             (W_dec) g = c w_j with live moments: the projection leaves pure cancellation.  (W_encT, b_enc: ``mixed``)
  orthogonal           (W_dec) w_j and g on a binary grid, column pairs (a, b) against s (b, -a): g . w = 0 exactly in any order
  one_hot_column       one non-zero gradient element, m = v = 0: in the last valid column d_in - 1 (first and last row of the class) and
                       in the columns 256 i - 1 / 256 i of every vector boundary below d_in (the seven rows between; beyond 1024 there
                       are eight such columns: the W_encT rows take all but 1024, the W_dec rows all but 255)
  mixed                randn g, moments with m^2 <= v
b_enc[j] follows its row's class, b_dec[i] the class of i % 8 (the row-only classes as ``mixed``).
Every non-zero g~^2, (1 - b2) g~^2 and v' lies in [2^-100, 2^100] (``assert_magnitudes``; g~ the clipped and projected gradient), so no
flush-to-zero or overflow mode of the hardware can matter.  The one exception is stated there: an element of a W_dec row whose projection
cancels to within its own error bound, where the bound's own term is asserted to stand far above anything a flush could drop.

Clip settings (``CLIPS``), all through the planted scalars[3], never through the gradient's own norm: ``disabled`` (max_grad_norm <= 0,
scalars[3] = 3 must be ignored), ``inactive`` (norm 0.5 < max 1), ``active`` (coef ~ 2^-7), ``zero_sq`` (scalars[3] = 0: coef = min(1e6, 1)),
``tiny`` (sqrt(scalars[3]) = max_grad_norm = 1e-6: the + 1e-6 of clip_grad_norm_ halves the coefficient).  Steps 1, 2, 1000, 100000.

The ``zero`` rows of W_encT carry the weight classes of the shadows (``WEIGHT_ROWS``; the value after the update is the planted one): exact
fp16 values, round-to-nearest-even ties (1 + 2^-11, 1 + 3 2^-11), fp16 subnormals and ties between them, 2^-24 / 2^-25 (the tie to zero) /
2^-26, and 60000 (the largest magnitude that is not ``big``).  ``big=True`` plants 60001, 65504, 65519, 65520 (rounds to fp16 inf), -65520,
NaN and +inf into one row each (``BIG_ROWS``; that row's g, m, v are zero).

The reference and the bounds (``reference``)
--------------------------------------------
float64 of oracle/sae_oracle.py's ``clip_and_project`` + ``adam_step`` with the coefficient from the planted scalars[3], on the pending-renorm
row rn w where a renorm is pending.  u = 2^-24, gamma(m) = m u / (1 - m u).  The build has -ffp-contract=off and HIP's default correctly
rounded fp32 divide and sqrt: every operation rounds once, relative u.  Per element, operation by operation:
  coef      t = sqrt(sq): u t;  t + 1e-6f: that + the constant's K_1EM6 1e-6 + u;  max / .: relative + u;  fminf: exact, and exactly 1 once
            the quotient's interval lies above 1
  rn w      u |rn w|;   g~ = coef g: |g| coef_err + u |g~|
  dot       gamma(d + 1) sum |g~ w| + sum (g~_err |w| + |g~| w_err)   (at most 4 V4 + 6 <= d + 1 operations in a lane and the butterfly)
  g~ - dot w   g~_err + dot_err |w| + |dot| w_err + u |dot w| + u |.|
  m'        a = g~ - m: g~_err + u |a|;  a c1: that c1 + |a| c1 (K_C1 + u);  m + .: + u |m'|
  v'        |v| b2 (K_B2 + u) + c2 g~^2 (K_C2 + 2 u) + c2 (2 |g~| g~_err + g~_err^2)(1 + K_C2) + u v'
  Delta     = (lr / bc1) m' / (sqrt(v') / bc2s + eps) is monotone in m' and in v': its input error is the largest deviation over the four
            corners (m' +- m'_err, max(v' +- v'_err, 0)) -- the exact form of "propagate through the partial derivatives", and still a
            bound where g~ lies within its error of 0 (first step: Delta = lr sign(g~)); the roundings with exact inputs are relative to
            |Delta| because the denominator is a sum of positive terms: sqrt u, / bc2s K_CAST + u, + eps K_EPS + u, m' / . u,
            lr / bc1 K_CAST + u, the product u  ->  ROUND_DELTA = 6 u + 2 K_CAST + K_EPS
  w - Delta w_err + Delta_err + u |w'|
The kernels' fp32 constants against the reference's double ones (K_*, computed below from the number formats, nothing measured):
  1.f - 0.9f   = 0.100000024 exactly (the subtraction is exact), 0.1 (1 + 4.0 u)        -> K_C1 = 2.4e-7
  1.f - 0.999f = 0.000999987125 exactly, 0.001 (1 - 216 u): the float nearest 0.999 lies 1.29e-8 above it, and that absolute
                 difference is 1.29e-5 of 0.001                                         -> K_C2 = 1.29e-5 (the largest term of every bound of v)
  0.999f       = 0.999 (1 + 0.22 u)  -> K_B2;   1e-8f = 1e-8 (1 - 0.10 u) -> K_EPS;   1e-6f = 1e-6 (1 - 0.43 u) -> K_1EM6
  (float)bc1, (float)bc2_sqrt: one rounding of the double the reference uses            -> K_CAST = u
Shadows, from the float32 row actually written (``got``): enc_colsq gamma(d + 6) sum w^2;  dec_inv_norm: that through 1 / sqrt(.):
inv (gamma(d + 6) / 2 + 2 u) (1 + gamma).  Sums of squares (``sqnorm_bound``): gamma(depth) sum g^2, depth = the longest chain of
operations a term passes through (its square, its thread's additions, the reduction's stages).  ``SECOND_ORDER`` covers the rest.

``check`` returns the worst error / bound per quantity -- inf for NaN where a number belongs -- and messages naming feature row, row class,
column and element; ``passes``: every ratio <= 1.

``twin``: a float32 numpy port of the kernels' structure (the row kernels' V4 vectors of 4 x 64 lanes and their butterfly, the 32 x 64 tile
walk with its transpose into W_enc, one ``big`` flag per thread of the tile form and per row of the row form, the bias vectors in a launch
of 256-element blocks); ``SLIPS`` are the wrong versions of it.
"""
import math

import numpy as np

F32, F64, F16 = np.float32, np.float64, np.float16
U = 2.0 ** -24
SECOND_ORDER = 1.0 + 2.0 ** -10
D_SAE = 72
WIDTHS = (64, 100, 256, 260, 768, 772, 1024, 1028, 1280)
STEPS = (1, 2, 1000, 100000)
ROW_CLASSES = ("zero", "zero_g_live_moments", "first_step", "eps_regime", "parallel", "orthogonal", "one_hot_column", "mixed")
ZERO, LIVE, FIRST, EPSR, PARALLEL, ORTH, ONEHOT, MIXED = range(8)
# name -> (max_grad_norm, scalars[3]); float32 values, the reference takes them as they are
CLIPS = {"disabled": (F32(0.0), F32(3.0)), "inactive": (F32(1.0), F32(0.25)), "active": (F32(1.0), F32(16461.0)),
         "zero_sq": (F32(1.0), F32(0.0)), "tiny": (F32(1e-6), F32(F32(1e-6) * F32(1e-6)))}
# the covering set of (d_in, clip, step) the apply tests run: every width once with the clips and steps cycling, every clip at the
# width that is ragged inside the first vector, every step at the width with one live lane in the last vector, the plan's maximum clipped
COVER = ((64, "disabled", 1), (100, "active", 2), (256, "inactive", 1000), (260, "tiny", 100000), (768, "zero_sq", 1), (772, "active", 1000),
         (1024, "disabled", 2), (1028, "inactive", 100000), (1280, "active", 1),
         (100, "disabled", 1000), (100, "inactive", 1), (100, "zero_sq", 100000), (100, "tiny", 1000),
         (260, "active", 1), (260, "active", 2), (260, "active", 1000), (1280, "tiny", 2))
WEIGHT_ROWS = {0: "fp16_exact", 8: "ties", 16: "subnormals", 24: "tiny", 32: "largest_not_big", 40: "subnormals", 48: "tiny", 56: "fp16_exact",
               64: "ties"}
BIG_ROWS = {3: 60001.0, 13: 65504.0, 33: math.inf, 38: 65519.0, 47: 65520.0, 66: -65520.0, 69: math.nan}
ELEMENTWISE = ("b_enc", "b_dec", "b_dec_out", "W_skip", "b_gate", "r_mag", "b_mag")
B1, B2, EPS = 0.9, 0.999, 1e-8


def _rel(f32_value, dbl):
    return abs(float(f32_value) - dbl) / abs(dbl)


K_C1 = _rel(F32(1) - F32(0.9), 1.0 - B1)
K_C2 = _rel(F32(1) - F32(0.999), 1.0 - B2)
K_B2 = _rel(F32(0.999), B2)
K_EPS = _rel(F32(1e-8), EPS)
K_1EM6 = _rel(F32(1e-6), 1e-6)
K_CAST = U
ROUND_DELTA = 6 * U + 2 * K_CAST + K_EPS
assert 3.9 * U < K_C1 < 4.1 * U and 215 * U < K_C2 < 217 * U and K_B2 < U and K_EPS < U and K_1EM6 < U


def gamma(m):
    m = np.asarray(m, F64)
    return m * U / (1.0 - m * U)


def v4_of(d):
    """V4_DISPATCH of csrc/sae.hpp"""
    return 1 if d <= 256 else 3 if d <= 768 else 4 if d <= 1024 else 5


def dpl_of(d):
    """DPL_DISPATCH of csrc/sae_apply.hip"""
    return 4 if d <= 256 else 12 if d <= 768 else 16 if d <= 1024 else 20


def _rng(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + (sum(map(ord, k)) if isinstance(k, str) else int(k))) % (2 ** 31)
    return np.random.RandomState(seed)


class Case:
    """P, G, M, V: float32 dicts over W_encT [d_sae, d_in] (the transposed encoder: the layout Adam runs in), W_dec, b_enc, b_dec (+ the
    transcoder's b_dec_out / W_skip or the gated b_gate / r_mag / b_mag); sq = scalars[3]; inv_norm [d_sae] or None: a pending decoder
    renorm; cls [d_sae]: the row classes; big {row: (column, value)}."""

    def __init__(self, name, P, G, M, V, sq, step, lr, max_grad_norm, j_lo, j_hi, inv_norm=None, cls=None, big=None, clip=None):
        self.name, self.P, self.G, self.M, self.V = name, P, G, M, V
        self.sq, self.step, self.lr, self.max_grad_norm = sq, int(step), lr, max_grad_norm      # (as given: float32 values for a kernel's call)
        self.d_sae, self.d_in = P["W_dec"].shape
        self.j_lo, self.j_hi = int(j_lo), int(self.d_sae if j_hi is None else j_hi)
        self.inv_norm, self.big, self.clip = inv_norm, dict(big or {}), clip
        self.G_err = {}                                                         # {key: bound of the given gradient's own error} (default: exact)
        self.cls = np.arange(self.d_sae) % 8 if cls is None else cls

    def row_class(self, j):
        return ROW_CLASSES[int(self.cls[j])]

    def __repr__(self):
        return f"<apply case {self.name} d_in={self.d_in} clip={self.clip} step={self.step} rows=[{self.j_lo}, {self.j_hi})>"


def coef64(max_grad_norm, sq):
    """-> (the float64 coefficient, the bound of the fp32 computation's error)"""
    mx = float(max_grad_norm)
    if not mx > 0:
        return 1.0, 0.0
    t = math.sqrt(float(sq))
    t_err = U * t
    t2 = t + 1e-6
    t2_err = t_err + K_1EM6 * 1e-6 + U * t2
    q = mx / t2
    q_err = q * t2_err / (t2 - t2_err) + U * q
    if q - q_err >= 1.0:
        return 1.0, 0.0                                                         # fminf gives exactly 1
    return min(q, 1.0), q_err


def one_hot_columns(d_in):
    inner = [c for i in range(1, 5) for c in (256 * i - 1, 256 * i) if c < d_in - 1]
    return [d_in - 1] + inner


def _plant(rs, k, shape, coef, step):
    """g, m, v (float64) of the elementwise classes; the row-only classes come out as ``mixed``"""
    k = np.broadcast_to(k, shape)
    g, m, v = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    sgn = rs.choice([-1.0, 1.0], size=shape)
    mm = 1e-2 * rs.standard_normal(shape)
    s = k == LIVE
    m[s], v[s] = mm[s], (mm ** 2 * (1.0 + rs.random_sample(shape)))[s]
    s = k == FIRST
    g[s] = (sgn * 2.0 ** rs.uniform(-20, 10, size=shape))[s]
    bc2 = 1.0 - B2 ** step
    vt = (1e-8 * 2.0 ** rs.uniform(-2.5, 2.5, size=shape)) ** 2 * bc2
    s = k == EPSR
    v[s] = (0.5 * vt / B2)[s]
    g[s] = (sgn * np.sqrt(0.5 * vt / (1.0 - B2)) / coef)[s]
    m[s] = (0.5 * np.sqrt(0.5 * vt / B2) * rs.choice([-1.0, 1.0], size=shape))[s]
    gm, m_ = rs.standard_normal(shape), 0.1 * rs.standard_normal(shape)
    s = (k == MIXED) | (k == PARALLEL) | (k == ORTH) | (k == ONEHOT)
    g[s], m[s], v[s] = gm[s], m_[s], (m_ ** 2 + 0.01 * rs.random_sample(shape))[s]
    return g, m, v


def _weight_row(kind, d_in, rs):
    if kind == "fp16_exact":
        return rs.randint(-2048, 2049, size=d_in) / 1024.0
    if kind == "ties":
        return rs.choice([-1.0, 1.0], size=d_in) * np.where(np.arange(d_in) % 2 == 0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11)
    if kind == "subnormals":                                                   # k 2^-24 and the ties (k + 1/2) 2^-24 between them
        k = rs.randint(1, 1024, size=d_in) + np.where(np.arange(d_in) % 3 == 0, 0.5, 0.0)
        return rs.choice([-1.0, 1.0], size=d_in) * k * 2.0 ** -24
    if kind == "tiny":
        return rs.choice([-1.0, 1.0], size=d_in) * 2.0 ** -(24.0 + np.arange(d_in) % 3)
    if kind == "largest_not_big":
        w = rs.randint(-2048, 2049, size=d_in) / 1024.0
        w[0], w[d_in - 1] = -60000.0, 60000.0
        return w
    raise KeyError(kind)


def make(d_in, clip="inactive", step=1, j_lo=0, j_hi=None, seed=0, big=False, pending=False, extras=None, d_sae=D_SAE):
    """pending: the W_dec rows at norms 2^-10 .. 2^10 with their inverse norms handed to apply (a deferred set_decoder_norm_to_unit_norm).
    extras: None, "transcoder" (b_dec_out, W_skip) or "gated" (b_gate, r_mag, b_mag), planted with the elementwise classes."""
    rs = _rng("apply", d_in, clip, step, seed, int(pending))
    max_norm, sq = CLIPS[clip]
    coef = coef64(max_norm, sq)[0]
    cls = np.arange(d_sae) % 8
    rowk = cls[:, None]
    W_dec = rs.uniform(-1.0, 1.0, size=(d_sae, d_in))
    W_dec /= np.linalg.norm(W_dec, axis=1, keepdims=True)
    W_encT = rs.standard_normal((d_sae, d_in)) / math.sqrt(d_in)
    P = dict(W_encT=W_encT, W_dec=W_dec, b_enc=0.01 * rs.standard_normal(d_sae), b_dec=0.05 * rs.standard_normal(d_in))
    G, M, V = {}, {}, {}
    for key, k, shape in (("W_encT", rowk, (d_sae, d_in)), ("W_dec", rowk, (d_sae, d_in)), ("b_enc", cls, (d_sae,)),
                          ("b_dec", np.arange(d_in) % 8, (d_in,))):
        G[key], M[key], V[key] = _plant(rs, k, shape, coef, step)
    if extras == "transcoder":
        P["b_dec_out"], P["W_skip"] = 0.05 * rs.standard_normal(d_in), rs.standard_normal((d_in, d_in)) / math.sqrt(d_in)
        for key, shape in (("b_dec_out", (d_in,)), ("W_skip", (d_in, d_in))):
            k = (np.arange(int(np.prod(shape))) % 8).reshape(shape)
            G[key], M[key], V[key] = _plant(rs, k, shape, coef, step)
    elif extras == "gated":
        for key in ("b_gate", "r_mag", "b_mag"):
            P[key] = 0.1 * rs.standard_normal(d_sae)
            G[key], M[key], V[key] = _plant(rs, cls, (d_sae,), coef, step)
    else:
        assert extras is None
    # the row-only classes
    scale = 2.0 ** -round(math.log2(math.sqrt(d_in) * 0.35))
    cols = one_hot_columns(d_in)
    hot_rows = np.flatnonzero(cls == ONEHOT)
    for j in range(d_sae):
        if cls[j] == ORTH:
            a = rs.randint(1, 9, size=d_in // 2) / 16.0 * rs.choice([-1.0, 1.0], size=d_in // 2)
            b = rs.randint(1, 9, size=d_in // 2) / 16.0 * rs.choice([-1.0, 1.0], size=d_in // 2)
            s_ = rs.randint(1, 9, size=d_in // 2) / 8.0 * rs.choice([-1.0, 1.0], size=d_in // 2)
            W_dec[j, 0::2], W_dec[j, 1::2] = a * scale, b * scale
            G["W_dec"][j, 0::2], G["W_dec"][j, 1::2] = s_ * b, -s_ * a
        elif cls[j] == ONEHOT:
            r = int(np.searchsorted(hot_rows, j))
            for key, shift in (("W_encT", 0), ("W_dec", 1 if len(cols) - 1 > len(hot_rows) - 2 else 0)):
                col = cols[0] if r in (0, len(hot_rows) - 1) or len(cols) == 1 else cols[1 + (r - 1 + shift) % (len(cols) - 1)]
                G[key][j], M[key][j], V[key][j] = 0.0, 0.0, 0.0
                G[key][j, col] = rs.choice([-1.0, 1.0]) * 2.0 ** rs.randint(-3, 4)
        elif cls[j] == ZERO and j in WEIGHT_ROWS:
            W_encT[j] = _weight_row(WEIGHT_ROWS[j], d_in, rs)
    planted_big = {}
    if big:
        for i, (j, val) in enumerate(sorted(BIG_ROWS.items())):
            if j >= d_sae:
                continue
            col = (d_in - 1, 0, d_in // 2)[i % 3]
            W_encT[j, col] = val
            planted_big[j] = (col, val)
            for D_ in (G, M, V):
                D_["W_encT"][j] = 0.0
    inv_norm = None
    if pending:
        e = (np.arange(d_sae) * 5) % 21 - 10
        assert set(e.tolist()) == set(range(-10, 11))
        W_dec *= 2.0 ** e[:, None]
    to32 = lambda D_: {k_: np.ascontiguousarray(v_, F32) for k_, v_ in D_.items()}
    P, G, M, V = to32(P), to32(G), to32(M), to32(V)
    if pending:
        inv_norm = (1.0 / np.sqrt((P["W_dec"].astype(F64) ** 2).sum(axis=1))).astype(F32)
    # the parallel rows: g = c (rn w) of the float32 row, live moments at the gradient's scale
    for j in np.flatnonzero(cls == PARALLEL):
        c_ = rs.choice([-1.0, 1.0]) * 2.0 ** rs.uniform(-3, 3)
        rn = float(inv_norm[j]) if pending else 1.0
        G["W_dec"][j] = (c_ * rn * P["W_dec"][j].astype(F64)).astype(F32)
        m_ = 0.1 * abs(c_) / math.sqrt(d_in) * rs.standard_normal(d_in)
        M["W_dec"][j], V["W_dec"][j] = m_.astype(F32), (m_ ** 2 + c_ ** 2 / d_in * (0.5 + rs.random_sample(d_in))).astype(F32)
    for key in V:                                                               # m^2 <= v survives the rounding to float32
        V[key] = np.maximum(V[key], (M[key].astype(F64) ** 2 * (1 + 4 * U)).astype(F32), dtype=F32)
    name = f"d{d_in}_{clip}_s{step}" + ("_big" if big else "") + ("_pending" if pending else "") + (f"_{extras}" if extras else "")
    return Case(name, P, G, M, V, sq, step, F32(1e-3), max_norm, j_lo, j_hi, inv_norm, cls, planted_big, clip)


# ------------------------------------------------------------------------------------------------------------ float64 reference
def _adam64(w, w_err, g, g_err, m, v, step, lr):
    """the elementwise Adam update in float64 and the bounds of m', v', w' (see the module docstring)"""
    bc1, bc2s = 1.0 - B1 ** step, math.sqrt(1.0 - B2 ** step)
    c1, c2 = 1.0 - B1, 1.0 - B2
    a = g - m
    m1 = m + a * c1
    a_err = g_err + U * np.abs(a)
    moved = (a != 0) | (g_err > 0)
    m_err = np.where(moved, a_err * c1 + np.abs(a) * c1 * (K_C1 + U) + U * np.abs(m1), 0.0)
    v1 = v * B2 + c2 * g * g
    v_err = np.abs(v) * B2 * (K_B2 + U) + c2 * g * g * (K_C2 + 2 * U) + c2 * (2 * np.abs(g) * g_err + g_err ** 2) * (1 + K_C2) + U * v1
    v_err = np.where((v != 0) | (g != 0) | (g_err > 0), v_err, 0.0)

    def delta(mm, vv):
        return (lr / bc1) * (mm / (np.sqrt(vv) / bc2s + EPS))

    D = delta(m1, v1)
    dev, dmax = np.zeros_like(D), np.abs(D)
    for mm in (m1 - m_err, m1 + m_err):
        for vv in (np.maximum(v1 - v_err, 0.0), v1 + v_err):
            c_ = delta(mm, vv)
            dev, dmax = np.maximum(dev, np.abs(c_ - D)), np.maximum(dmax, np.abs(c_))
    D_err = dev + ROUND_DELTA * dmax
    w1 = w - D
    w1_err = w_err + D_err + np.where((D_err > 0) | (w_err > 0), U * np.abs(w1), 0.0)
    return dict(w=w1, w_bound=w1_err, m=m1, m_bound=m_err, v=v1, v_bound=v_err, delta=D)


def reference(c):
    """-> {key: the float64 parameter after the apply, key_bound, m_key, m_key_bound, v_key, v_key_bound} over the FULL arrays: outside
    [j_lo, j_hi) the value is the input and the bound 0 (b_dec and the extra tensors move on every call); coef, coef_err; gt_<key>: the
    clipped and projected gradient of the rows applied."""
    coef, coef_err = coef64(c.max_grad_norm, c.sq)
    clip_on = float(c.max_grad_norm) > 0
    lr, step = float(c.lr), c.step
    sl = slice(c.j_lo, c.j_hi)
    r = dict(coef=coef, coef_err=coef_err)
    for key in c.P:
        P, G, M, V = (D_[key].astype(F64) for D_ in (c.P, c.G, c.M, c.V))
        rows = sl if key in ("W_encT", "W_dec", "b_enc") else slice(None)
        w, g, m, v = P[rows], G[rows], M[rows], V[rows]
        w_err = np.zeros_like(w)
        if key == "W_dec" and c.inv_norm is not None:
            w = w * c.inv_norm.astype(F64)[rows, None]
            w_err = U * np.abs(w)
        gt = coef * g
        gt_err = (np.abs(g) * coef_err + U * np.abs(gt)) if clip_on else np.zeros_like(g)
        if key in c.G_err:                                                      # the gradient is a kernel's own: the reference's, within this
            gt_err = gt_err + (coef + coef_err) * np.asarray(c.G_err[key], F64)[rows]
        if key == "W_dec":
            d = w.shape[1]
            dot = (gt * w).sum(axis=1, keepdims=True)
            dot_err = gamma(d + 1) * (np.abs(gt * w)).sum(axis=1, keepdims=True) + (gt_err * np.abs(w) + np.abs(gt) * w_err).sum(axis=1, keepdims=True)
            gp = gt - dot * w
            gp_err = gt_err + dot_err * np.abs(w) + np.abs(dot) * w_err + U * np.abs(dot * w) + U * np.abs(gp)
            gp_err = np.where((dot_err > 0) | (dot != 0), gp_err, gt_err)
            r["dot"], r["dot_err"] = dot[:, 0], dot_err[:, 0]
            gt, gt_err = gp, gp_err
        a = _adam64(w, w_err, gt, gt_err, m, v, step, lr)
        for q_, src, pre in (("w", P, ""), ("m", M, "m_"), ("v", V, "v_")):
            full, bound = src.copy(), np.zeros_like(src)
            full[rows], bound[rows] = a[q_], a[q_ + "_bound"] * SECOND_ORDER
            r[pre + key], r[pre + key + "_bound"] = full, bound
        r["gt_" + key], r["gt_err_" + key] = gt, gt_err
    return r


def assert_magnitudes(c, ref=None):
    """every non-zero g~^2, (1 - b2) g~^2 and v' in [2^-100, 2^100]; the one exception: an element of a W_dec row whose projection cancels
    to within its own error bound g~_err -- what the kernel holds there may be anything in [-2 g~_err, 2 g~_err], arbitrarily small; there
    the term (1 - b2) g~_err^2 that the bound of v' carries is itself at least 2^-100, and what a flush could drop (below 2^-126) is
    invisible under it"""
    ref = ref or reference(c)
    lo, hi = 2.0 ** -100, 2.0 ** 100
    for key in c.P:
        g, ge = ref["gt_" + key], ref["gt_err_" + key]
        rows = slice(c.j_lo, c.j_hi) if key in ("W_encT", "W_dec", "b_enc") else slice(None)
        v1 = ref["v_" + key][rows]
        if key == "W_encT" and c.big:
            keep = np.ones(g.shape[0], bool)
            keep[[j - c.j_lo for j in c.big if c.j_lo <= j < c.j_hi]] = False
            g, ge, v1 = g[keep], ge[keep], v1[keep]
        noise = (np.abs(g) <= ge) & (g != 0)
        assert key == "W_dec" or not noise.any(), key
        assert ((1.0 - B2) * ge[noise] ** 2 >= lo).all(), key
        for t in (g * g, (1.0 - B2) * g * g):
            t = t[(g != 0) & ~noise]
            assert t.size == 0 or (t.min() >= lo and t.max() < hi), (key, t.min(), t.max())
        t = v1[v1 != 0]
        assert t.size == 0 or (t.min() >= lo and t.max() < hi), (key, t.min(), t.max())


def colsq_ref(WT_written):
    """enc_colsq of the float32 rows actually written, and its bound"""
    s = (np.asarray(WT_written, F64) ** 2).sum(axis=1)
    return s, gamma(WT_written.shape[1] + 6) * s * SECOND_ORDER


def inv_norm_ref(W_written):
    s = (np.asarray(W_written, F64) ** 2).sum(axis=1)
    g_ = gamma(W_written.shape[1] + 6)
    with np.errstate(divide="ignore"):
        inv = 1.0 / np.sqrt(s)
    return inv, inv * (g_ / 2 + 2 * U) * (1 + g_) * SECOND_ORDER


def renorm_ref(W):
    """set_decoder_norm_to_unit_norm of float32 rows: w / sqrt(sum w^2) -- the sum gamma(d + 6), the root u, the quotient u"""
    W = np.asarray(W, F64)
    out = W / np.sqrt((W ** 2).sum(axis=1, keepdims=True))
    g_ = gamma(W.shape[1] + 6)
    return out, np.abs(out) * (g_ / 2 + 2 * U) * (1 + g_) * SECOND_ORDER


def shadow_case(WT_expected, j_lo, j_hi):
    """a state whose every row is ``zero``: what ``check`` needs to hold the shadows of W_encT as it must stand after a sync_shadows of
    [j_lo, j_hi) -- the copies bit for bit, enc_colsq to its bound and to the ``big`` rule"""
    WT = np.ascontiguousarray(WT_expected, F32)
    d_sae, d_in = WT.shape
    z = lambda: dict(W_encT=np.zeros((d_sae, d_in), F32), W_dec=np.zeros((d_sae, d_in), F32), b_enc=np.zeros(d_sae, F32), b_dec=np.zeros(d_in, F32))
    big = {int(j): (int(np.flatnonzero(~(np.abs(WT[j].astype(F64)) <= 6.0e4))[0]),) * 2 for j in np.flatnonzero(big_rows(WT))}
    big = {j: (col, float(WT[j, col])) for j, (col, _) in big.items()}
    return Case("shadows", dict(z(), W_encT=WT), z(), z(), z(), F32(0), 1, F32(1e-3), F32(0), j_lo, j_hi, cls=np.zeros(d_sae, np.int64), big=big)


def big_rows(WT_written):
    """rows holding an element beyond 6.0e4 or a non-finite one: enc_colsq = +inf is mandatory"""
    return ~(np.abs(np.asarray(WT_written, F64)) <= 6.0e4).all(axis=1)


def sqnorm_depth(n, grid=1024):
    """sqnorm_partial_kernel on `grid` workgroups + reduce_sum_kernel over the 1024-float partial array: a term's square, its thread's 4
    additions per sweep of grid x 1024 elements, the butterfly and the four waves of block_sum_256 (6 + 3), the reduction's own thread
    (one addition into one of four accumulators, two to combine them) and block sum"""
    return 1 + 4 * (-(-n // (grid * 1024))) + 9 + 3 + 9


def sqnorm_bound(terms, depth):
    s = float((np.asarray(terms, F64) ** 2).sum())
    return s, float(gamma(depth)) * s * SECOND_ORDER


# ------------------------------------------------------------------------------------------------------------ the checker
def _ratios(got, ref, bound):
    got = np.asarray(got, F64)
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.abs(got - ref)
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return np.where(np.isfinite(got), r, np.inf)


def check(c, ref, got, form="tile"):
    """got: W_encT, W_dec, b_enc, b_dec (+ extras), m_<key>, v_<key>: what the apply left (full arrays); optional W_enc [d_in, d_sae], W_enc16T
    (float16), enc_colsq, dec_inv_norm, each with ``<name>_before`` (what it held before the call: rows outside [j_lo, j_hi) must keep their
    bits).  form: "tile" (wenc_rows_kernel: enc_colsq may be +inf for the rows that share a thread with a ``big`` row -- same 32-row tile counted
    from j_lo, same row mod 8) or "rows" (adam_wenct_kernel: it may not).
    -> (ratios {quantity: worst error / bound; exact checks: 0 or inf; conservative_inf: the count of finite rows reported +inf}, messages)"""
    ratios, msgs = {}, []
    lo, hi = c.j_lo, c.j_hi
    inside = np.zeros(c.d_sae, bool)
    inside[lo:hi] = True
    nonfinite = np.array(sorted(j for j, (_, v_) in c.big.items() if not math.isfinite(v_)), np.int64)

    def exact(name, ok, what):
        ratios[name] = 0.0 if ok else math.inf
        if not ok:
            msgs.append(f"{name}: {what() if callable(what) else what}")

    def where(key, w):
        if key in ("W_encT", "W_dec"):
            return f"feature row {w[0]} (class {c.row_class(w[0])}) column {w[1]} element {tuple(w)}"
        if key == "b_enc" or key in ("b_gate", "r_mag", "b_mag"):
            return f"feature row {w[0]} (class {c.row_class(w[0])}) element {tuple(w)}"
        return f"element {tuple(w)} (class {ROW_CLASSES[int(np.ravel_multi_index(w, c.P[key].shape)) % 8]})"

    for key in c.P:
        for pre in ("", "m_", "v_"):
            name = pre + key
            if name not in got:
                continue
            g = np.asarray(got[name], F64)
            r = _ratios(g, ref[name], ref[name + "_bound"])
            if key == "W_encT" and nonfinite.size and pre == "":               # a planted NaN / inf row: only that it is still there
                bad = [j for j in nonfinite if np.isfinite(g[j, c.big[j][0]])]
                exact("nonfinite_rows_kept", not bad, f"feature row {bad[:1]}: the planted non-finite weight is gone")
                r[nonfinite] = 0.0
            worst = float(r.max()) if r.size else 0.0
            ratios[name] = worst
            if not worst <= 1.0:
                w = tuple(int(i) for i in np.unravel_index(int(np.argmax(np.where(np.isnan(r), np.inf, r))), r.shape))
                msgs.append(f"{name}: {where(key, w)}: got {g[w]!r}, float64 {ref[name][w]!r}, bound {ref[name + '_bound'][w]:.3e}, "
                            f"ratio {worst:.3g}" + ("" if key not in ("W_encT", "W_dec", "b_enc") or inside[w[0]] else " (outside the range applied)"))
    zero = np.flatnonzero((c.cls == ZERO))
    for key in ("W_encT", "W_dec"):
        if key in got:
            rows = [j for j in zero if not (key == "W_dec" and c.inv_norm is not None) and j not in nonfinite]
            same = [j for j in rows if not np.array_equal(np.asarray(got[key])[j].view(np.int32), c.P[key][j].view(np.int32))]
            exact(f"{key}_zero_rows", not same, lambda: f"feature row {same[0]} (class zero) changed bits")
    WT = np.asarray(got["W_encT"], F32) if "W_encT" in got else None
    if "W_enc" in got:
        W = np.asarray(got["W_enc"], F32)
        bad = np.argwhere(W.T.view(np.int32) != WT.view(np.int32))
        exact("W_enc", bad.size == 0, lambda: f"feature row {bad[0][0]} (class {c.row_class(bad[0][0])}) column {bad[0][1]}: W_enc is not W_encT transposed")
    if "W_enc16T" in got:
        h = np.asarray(got["W_enc16T"])
        with np.errstate(over="ignore", invalid="ignore"):
            want = WT.astype(F16)
        if "W_enc16T_before" in got:
            want[~inside] = np.asarray(got["W_enc16T_before"])[~inside]
        fin = np.ones(c.d_sae, bool)
        fin[nonfinite] = False
        bad = np.argwhere(h[fin].view(np.int16) != want[fin].view(np.int16))
        exact("W_enc16T", bad.size == 0, lambda: f"feature row {np.flatnonzero(fin)[bad[0][0]]} (class {c.row_class(np.flatnonzero(fin)[bad[0][0]])}) "
              f"column {bad[0][1]}: not W_encT rounded to fp16" + ("" if inside[np.flatnonzero(fin)[bad[0][0]]] else " (outside the range applied)"))
    if "enc_colsq" in got:
        q = np.asarray(got["enc_colsq"], F64)
        s, b = colsq_ref(WT)
        must = big_rows(WT) & inside
        may = np.zeros(c.d_sae, bool)
        if form == "tile":
            for j in np.flatnonzero(must):
                t0 = lo + (j - lo) // 32 * 32
                may[[i for i in range(t0, min(t0 + 32, hi)) if (i - j) % 8 == 0]] = True
        missing = np.flatnonzero(must & ~(np.isinf(q) & (q > 0)))
        exact("enc_colsq_big", missing.size == 0, lambda: f"feature row {missing[0]} (class {c.row_class(missing[0])}) holds an element beyond 6.0e4 "
              f"or a non-finite one, enc_colsq = {q[missing[0]]!r} is not +inf")
        cons = inside & ~must & np.isinf(q) & (q > 0)
        wrong = np.flatnonzero(cons & ~may)
        exact("enc_colsq_conservative", wrong.size == 0, lambda: f"feature row {wrong[0]} (class {c.row_class(wrong[0])}) is finite and shares no "
              f"thread with a big row, enc_colsq = +inf")
        ratios["conservative_inf"] = float(cons.sum())
        held = inside & ~must & ~cons
        with np.errstate(invalid="ignore"):
            r = _ratios(q[held], s[held], b[held])
        ratios["enc_colsq"] = float(r.max()) if r.size else 0.0
        if not ratios["enc_colsq"] <= 1.0:
            j = int(np.flatnonzero(held)[int(np.argmax(np.where(np.isnan(r), np.inf, r)))])
            msgs.append(f"enc_colsq: feature row {j} (class {c.row_class(j)}): got {q[j]!r}, float64 of the row written {s[j]!r}, bound {b[j]:.3e}, "
                        f"ratio {ratios['enc_colsq']:.3g}")
        if "enc_colsq_before" in got:
            out = np.flatnonzero(~inside & (np.asarray(got["enc_colsq"]).view(np.int32) != np.asarray(got["enc_colsq_before"]).view(np.int32)))
            exact("enc_colsq_outside", out.size == 0, lambda: f"feature row {out[0]} outside the range applied was written")
    if "dec_inv_norm" in got:
        q = np.asarray(got["dec_inv_norm"], F64)
        inv, b = inv_norm_ref(np.asarray(got["W_dec"], F32))
        r = _ratios(q[inside], inv[inside], b[inside])
        ratios["dec_inv_norm"] = float(r.max()) if r.size else 0.0
        if not ratios["dec_inv_norm"] <= 1.0:
            j = int(np.flatnonzero(inside)[int(np.argmax(np.where(np.isnan(r), np.inf, r)))])
            msgs.append(f"dec_inv_norm: feature row {j} (class {c.row_class(j)}): got {q[j]!r}, float64 of the row written {inv[j]!r}, bound {b[j]:.3e}, "
                        f"ratio {ratios['dec_inv_norm']:.3g}")
        if "dec_inv_norm_before" in got:
            out = np.flatnonzero(~inside & (np.asarray(got["dec_inv_norm"]).view(np.int32) != np.asarray(got["dec_inv_norm_before"]).view(np.int32)))
            exact("dec_inv_norm_outside", out.size == 0, lambda: f"feature row {out[0]} outside the range applied was written")
    return ratios, msgs


def passes(ratios):
    return all(v <= 1.0 for k_, v in ratios.items() if k_ != "conservative_inf")


def fmt(ratios):
    return " ".join(f"{k_}={v:.3g}" for k_, v in ratios.items())


# ------------------------------------------------------------------------------------------------------------ the float32 twin
SLIPS = ("coef_without_1e-6", "coef_left_out_of_the_dot", "dot_with_the_unrenormed_row", "projection_skipped_in_the_last_ragged_vector",
         "last_valid_vector_not_written", "bias_correction_from_step_minus_1", "eps_inside_the_square_root", "zero_g_live_moments_rows_skipped",
         "row_j_hi_touched", "row_j_hi_minus_1_skipped", "b_enc_range_taken_from_0", "W_enc16T_from_the_old_weight", "enc_colsq_from_the_old_weight",
         "enc_colsq_without_the_big_rule", "big_threshold_at_65504", "transposed_write_drops_the_ragged_rows", "dec_inv_norm_from_the_row_before",
         "tail_block_of_a_vector_kernel_dropped")


def _butterfly(x):
    """wave_sum / the tile form's 32-lane sum: v += shfl_xor(v, o) for o = width / 2 .. 1, over the last axis"""
    idx = np.arange(x.shape[-1])
    o = x.shape[-1] // 2
    while o:
        x = (x + x[..., idx ^ o]).astype(F32)
        o //= 2
    return x[..., 0]


def _lanes(a, V4):
    """[rows, d] -> [rows, V4, 64, 4] zero padded: vector i of lane l holds the columns 256 i + 4 l .. + 3"""
    rows, d = a.shape
    out = np.zeros((rows, 256 * V4), F32)
    out[:, :d] = a
    return out.reshape(rows, V4, 64, 4)


def _lane_dot(a, b, V4):
    """per lane: for i < V4: acc += a.x b.x + a.y b.y + a.z b.z + a.w b.w (left to right), then the butterfly"""
    A, B = _lanes(a, V4), _lanes(b, V4)
    acc = np.zeros((a.shape[0], 64), F32)
    for i in range(V4):
        p = A[:, i] * B[:, i]
        acc = acc + (((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3])
    return _butterfly(acc)


def twin(c, slip=None, lazy=False, fold=1):
    """pv_sae_apply in float32 as csrc/sae_apply.hip runs it.  lazy: the row form of the encoder (adam_wenct_kernel, W_enc == NULL: the parameter
    layout is left as it was); fold: the bias vectors ride in that launch (the same blocks either way).  -> what ``check`` takes, with the
    ``_before`` arrays as a fresh engine's sync_shadows leaves them."""
    assert slip is None or slip in SLIPS, slip
    f = F32
    d, d_sae, lo, hi = c.d_in, c.d_sae, c.j_lo, c.j_hi
    P = {k_: v_.copy() for k_, v_ in c.P.items()}
    M = {k_: v_.copy() for k_, v_ in c.M.items()}
    V = {k_: v_.copy() for k_, v_ in c.V.items()}
    G = c.G
    step = c.step - 1 if slip == "bias_correction_from_step_minus_1" else c.step
    bc1, bc2s = f(1.0 - 0.9 ** step), f(math.sqrt(1.0 - 0.999 ** step))
    lr, b1, b2, eps, one = f(c.lr), f(0.9), f(0.999), f(1e-8), f(1)
    if float(c.max_grad_norm) <= 0:
        coef = one
    else:
        total = np.sqrt(f(c.sq))
        coef = np.minimum(f(c.max_grad_norm) / (total if slip == "coef_without_1e-6" else total + f(1e-6)), one)
    coef = f(coef)

    def adam(w, g, m, v):
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            m1 = (m + (g - m) * (one - b1)).astype(F32)
            v1 = (v * b2 + (one - b2) * g * g).astype(F32)
            denom = (np.sqrt(v1 + eps) / bc2s) if slip == "eps_inside_the_square_root" else (np.sqrt(v1) / bc2s + eps)
            return (w - (lr / bc1) * (m1 / denom)).astype(F32), m1, v1

    with np.errstate(over="ignore", invalid="ignore"):
        W16 = P["W_encT"].astype(F16)
    W_enc = np.ascontiguousarray(P["W_encT"].T)
    colsq = np.zeros(d_sae, F32)
    for j0 in range(0, d_sae, 32):                                              # (what sync_shadows left)
        colsq[j0:j0 + 32] = _tile_colsq(P["W_encT"][j0:j0 + 32], None)
    inv = np.ones(d_sae, F32) if c.inv_norm is None else c.inv_norm.copy()
    before = dict(W_enc16T_before=W16.copy(), enc_colsq_before=colsq.copy(), dec_inv_norm_before=inv.copy())
    V4 = v4_of(d)
    r_hi = min(hi + 1, d_sae) if slip == "row_j_hi_touched" else hi - 1 if slip == "row_j_hi_minus_1_skipped" else hi
    rows = np.arange(lo, r_hi)
    if slip == "zero_g_live_moments_rows_skipped":
        rows_d = rows[(G["W_dec"][rows] != 0).any(axis=1)]
        rows_e = rows[(G["W_encT"][rows] != 0).any(axis=1)]
    else:
        rows_d = rows_e = rows
    # ---- adam_wdec_kernel: a wave per row
    if rows_d.size:
        w_old = P["W_dec"][rows_d]
        rn = inv[rows_d][:, None] if c.inv_norm is not None else one
        w = (w_old * rn).astype(F32)
        g = (G["W_dec"][rows_d] * coef).astype(F32)
        g_dot = G["W_dec"][rows_d] if slip == "coef_left_out_of_the_dot" else g
        dot = _lane_dot(g_dot, w_old if slip == "dot_with_the_unrenormed_row" else w, V4)[:, None]
        gp = (g - dot * w).astype(F32)
        if slip == "projection_skipped_in_the_last_ragged_vector" and d % 256:
            gp[:, 256 * (d // 256):] = g[:, 256 * (d // 256):]
        wn, m1, v1 = adam(w, gp, M["W_dec"][rows_d], V["W_dec"][rows_d])
        dw = d - 4 if slip == "last_valid_vector_not_written" else d
        P["W_dec"][rows_d, :dw], M["W_dec"][rows_d, :dw], V["W_dec"][rows_d, :dw] = wn[:, :dw], m1[:, :dw], v1[:, :dw]
        src = w if slip == "dec_inv_norm_from_the_row_before" else wn
        with np.errstate(divide="ignore"):
            inv[rows_d] = one / np.sqrt(_lane_dot(src, src, V4))
    # ---- the encoder: the tile form (wenc_rows_kernel<0>) or the row form (adam_wenct_kernel)
    if rows_e.size:
        w_old = P["W_encT"][rows_e]
        wn, m1, v1 = adam(w_old, (G["W_encT"][rows_e] * coef).astype(F32), M["W_encT"][rows_e], V["W_encT"][rows_e])
        P["W_encT"][rows_e], M["W_encT"][rows_e], V["W_encT"][rows_e] = wn, m1, v1
        with np.errstate(over="ignore", invalid="ignore"):
            W16[rows_e] = (w_old if slip == "W_enc16T_from_the_old_weight" else wn).astype(F16)
        src = w_old if slip == "enc_colsq_from_the_old_weight" else wn
        thr = f(65504.0) if slip == "big_threshold_at_65504" else f(6.0e4)
        if slip == "enc_colsq_without_the_big_rule":
            thr = None
        if lazy:
            with np.errstate(invalid="ignore", over="ignore"):
                sq = _lane_dot(src, src, V4)
                if thr is not None:
                    sq = np.where(~(np.abs(src) <= thr).all(axis=1), f(np.inf), sq)
            colsq[rows_e] = sq
        else:
            pos = {int(j): i for i, j in enumerate(rows_e)}
            for j0 in range(lo, r_hi, 32):
                tile = np.zeros((32, d), F32)
                present = [j for j in range(j0, min(j0 + 32, r_hi)) if j in pos]
                for j in present:
                    tile[j - j0] = src[pos[j]]
                cs = _tile_colsq(tile, thr, no_rule=thr is None)
                for j in present:
                    colsq[j] = cs[j - j0]
            i_hi = 64 * (d // 64) if slip == "transposed_write_drops_the_ragged_rows" else d
            W_enc[:i_hi, rows_e] = wn.T[:i_hi]
    # ---- the vectors: blocks of 256 elements
    b_lo, b_hi = (0, hi - lo) if slip == "b_enc_range_taken_from_0" else (lo, hi)
    spans = [("b_enc", b_lo, b_hi), ("b_dec", 0, d)] + [(k_, 0, P[k_].size) for k_ in ("b_dec_out", "W_skip", "b_gate", "r_mag", "b_mag") if k_ in P]
    for key, a, b in spans:
        if slip == "tail_block_of_a_vector_kernel_dropped":
            b = a + 256 * ((b - a) // 256)
        w, m, v, g = P[key].reshape(-1), M[key].reshape(-1), V[key].reshape(-1), G[key].reshape(-1)
        w[a:b], m[a:b], v[a:b] = adam(w[a:b], (g[a:b] * coef).astype(F32), m[a:b], v[a:b])
    out = dict(P)
    out.update({"m_" + k_: v_ for k_, v_ in M.items()})
    out.update({"v_" + k_: v_ for k_, v_ in V.items()})
    out.update(before, W_enc16T=W16, enc_colsq=colsq, dec_inv_norm=inv)
    out["W_enc_stale" if lazy else "W_enc"] = W_enc                              # (the row form leaves the parameter's own layout as it was)
    return out


def _tile_colsq(tile, thr, no_rule=False):
    """one 32-feature tile of wenc_rows_kernel: thread (tx, ty) owns the rows ty + 8 r, r < 4, and of each the columns = tx mod 32, summed
    in column order; ONE ``big`` flag per thread over its four rows; then the 32-lane butterfly per row.  thr None (and not no_rule): 6.0e4"""
    rows, d = tile.shape
    f = F32
    pad = np.zeros((32, 32 * (-(-d // 32))), F32)
    pad[:rows, :d] = tile
    with np.errstate(over="ignore", invalid="ignore"):
        sq = np.cumsum((pad * pad).reshape(32, -1, 32), axis=1, dtype=F32)[:, -1]      # [row, tx]
        if not no_rule:
            bigel = ~(np.abs(pad) <= (f(6.0e4) if thr is None else thr))
            bigel[:, d:] = False
            bigel[rows:] = False
            per_thread = bigel.reshape(4, 8, -1, 32).any(axis=(0, 2))                  # [ty, tx]: rows r * 8 + ty
            sq = np.where(np.tile(per_thread, (4, 1)), f(np.inf), sq)
        return _butterfly(sq)[:rows]
