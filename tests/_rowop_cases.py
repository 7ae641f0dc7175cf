"""Planted inputs for the row and elementwise kernels (LayerNorm, the MLP activation, the token mean, the L2 normalise), their float64
references and per-element bound checkers.  Plain torch / numpy on the CPU, importable without a GPU.

The GPU suite otherwise feeds these kernels what a synthetic ViT produces and judges them by a tensor-wide relative Frobenius norm (or
by 2^-8 of a row's largest entry), which one wrong row, one wrong 8-element chunk or a wrong negative tail of the activation passes
(tests/test_rowop_cases_cpu.py shows it).  Here every input is known, every reference is float64 and every bound is per element.

LayerNorm rows (``ln_rows``; bf16-exact fp32, the same values for both dtypes; row r of a [rows, d] block):
``normal``       N(0, 1)
``offset``       1000 + 4 {-1, 0, 1}, the three values in equal numbers: |mean| / scale about 300
``const``        one value across the row (a different one per row): x - mean is exactly 0, scale = sqrt(eps), the output is b.  The
                 values are multiples of 1/8 below 8, one row 0 and one 1000, so that the fp32 sum of two of them (the EMBED form's
                 row in fp32 mode, which is no bf16 value) still adds up 2048 times without a rounding
``massive``      N(0, 1), channel 0 = 180, channel d - 1 = -300
``outlier``      N(0, 1), one channel (151 r + 5 mod d: the register chunk changes from row to row) at 2^14
``onehot_last``  zeros, channel d - 1 = 1: the last lane of the last register chunk holds all there is
``tiny``         N(0, 1) 2^-40: eps dominates the scale
``huge``         N(0, 1) 2^50: the squares stay finite in fp32
``nonfinite``    ``normal``, but rows 1 and 6 of every 8 are bad, cycling over: one NaN; one +inf; one -inf; NaN, +inf and -inf
                 together.  Every 4-row workgroup of ln_kernel holds good rows beside a bad one.  A bad row's expectation is what
                 layer_norm.py:88-93 gives in torch fp32: NaN throughout, its scale included.
Weights (``ln_weights``): w = bf16(1 + 0.5 N(0, 1)), b = bf16(N(0, 1)), or the module's default w = 1, b = 0.

LayerNorm reference and bounds (``ln_reference``, ``check_ln``): float64 of layer_norm.py:88-93.  With xn = (x - mean) / scale,
amp = 1 + |mean| / scale and A = |xn w| + |b| + |w| amp (amp: the mean's rounding error carried into a small spread), u = 2^-24:
  hook_scale (fp32 in both dtypes)          |got - ref| <= 8 u ref
  fp32 hook_normalized / fp32 LN output     |got - ref| <= 8 u A              per element
  bf16 LN output                            |got - ref| <= 2^-8 |ref| + 8 u A per element
The 8 is not taken from the GPU: ``ln_twin``, a float32 emulation of ln_kernel's summation order (per lane sequential over its chunks,
the 6-step xor tree, true division), reaches 3.1 u on the scale and 2.3 u A on the elements over these cases, torch fp32 of the
reference's formula the same (tests/test_rowop_cases_cpu.py asserts both below 4); 8 leaves room for the hardware's sqrt and division.

Pre-activations: ``all_bf16`` the 65 536 bf16 bit patterns, ``finite_bf16`` the 65 280 finite ones, ``fp32_extra(n)`` fp32 values that
are not bf16-exact: uniform in bit pattern over |x| < 2^7, the last 4096 uniform in [-9, -3] where 1 + erf cancels.

Activation references (float64, accurate in the tail, of x as stored) and bounds (``act_reference``, ``act_bound``, ``check_act``):
  gelu        0.5 x erfc(-x / sqrt 2)          quick_gelu   x / (1 + exp(-1.702 x))          relu   max(x, 0), exact
  bf16        |got - ref| <= 2^-8 |ref| + 2^-23 |x| + 2^-126
  fp32 gelu   |got - ref| <= 2^-21 |ref| + 5.66 2^-23 |x| + 2^-126
  fp32 quick  |got - ref| <= (2^-21 + 2^-23 |1.702 x|) |ref| + 2^-23 |x| + 2^-126
The 2^-23 |x| term is one ulp of the fp32 sum 1 + erf (or of the sigmoid) times |x| / 2, doubled: torch's own fp32 GELU needs it (it
flushes gelu(x) to -0 below about -5.4).  2^-126 covers denormal results.  The |1.702 x| term is the argument scaling of an fp32 exp.
The fp32 gelu's 5.66 was 1 and had to move: torch's fp32 F.gelu itself needs 2.83 2^-23 |x| there (at x = -2.985 of 4 000 000 uniform
values in [-9, 0]; 2.26 on ``fp32_extra``: its erf is several ulp off where 1 + erf cancels), so the term is twice torch's figure.
torch's F.gelu also overflows to inf for x >= 2^127 (it forms x (1 + erf) before the 0.5), where the float64 reference, and act2, give x:
``TORCH_GELU_MAX`` bounds the inputs on which torch's own GELU is asked to meet these bounds.
Non-finite inputs: what the reference's formulas give in torch fp32 (``act_formula``): NaN -> NaN, +inf -> +inf, -inf -> 0 (relu) / NaN.
(The formula written out, not F.gelu: the vector path of torch's CPU F.gelu returns NaN for +inf in fp32 where its scalar path, its float64
and the formula 0.5 x (1 + erf(x / sqrt 2)) all give +inf.)

Every ``check_*`` returns the worst error / bound per quantity -- inf for what no finite ratio excuses: a NaN where a number belongs, a
number where NaN belongs, a value that was never written.  ``passes``: every ratio <= 1.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
BF16_EPS = 2.0 ** -8
LN_EPS = 1e-5
LN_FACTOR = 8.0
GELU_FP32_TAIL = 2 * 2.83 * 2.0 ** -23                  # twice torch fp32 F.gelu's own figure (module docstring)
TORCH_GELU_MAX = 2.0 ** 127
LN_CASES = ("normal", "offset", "const", "massive", "outlier", "onehot_last", "tiny", "huge", "nonfinite")
ACTS = ("gelu", "quick_gelu", "relu")
PV_ACT = {"gelu": 0, "quick_gelu": 1, "relu": 2}
UNWRITTEN = 7.0                                          # what a twin leaves where it does not store


def _bf16(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _gen(*key):
    seed = 0
    for k in key:
        seed = seed * 1000003 + (sum(map(ord, k)) if isinstance(k, str) else int(k))
    return torch.Generator().manual_seed(seed % (2 ** 31))


# ---------------------------------------------------------------------------------------------------------------- LayerNorm: inputs
def bad_ln_rows(rows):
    """nonfinite: the rows that hold a non-finite value"""
    return [r for r in range(rows) if r % 8 in (1, 6)]


def outlier_channel(r, d):
    return (151 * r + 5) % d


def ln_rows(name, rows, d, seed=0):
    """[rows, d] float32 on the CPU holding bf16-representable values"""
    assert name in LN_CASES and d % 8 == 0
    g = _gen("ln", "normal" if name == "nonfinite" else name, rows, d, seed)       # (nonfinite: the normal rows, some spoiled)
    x = torch.randn(rows, d, generator=g)
    r = torch.arange(rows)
    if name == "offset":
        k = torch.stack([(torch.randperm(d, generator=g) + i) % 3 for i in range(rows)])      # -1, 0, 1 in equal numbers (+-1)
        x = 1000.0 + 4.0 * (k.float() - 1.0)
    elif name == "const":
        x = (torch.round(24.0 * torch.randn(rows, 1, generator=g)).clamp(-63, 63) / 8.0).expand(rows, d).clone()
        x[0] = 0.0
        if rows > 2:
            x[2] = 1000.0
    elif name == "massive":
        x[:, 0], x[:, d - 1] = 180.0, -300.0
    elif name == "outlier":
        x[r, torch.tensor([outlier_channel(int(i), d) for i in r])] = 2.0 ** 14
    elif name == "onehot_last":
        x = torch.zeros(rows, d)
        x[:, d - 1] = 1.0
    elif name == "tiny":
        x = x * 2.0 ** -40
    elif name == "huge":
        x = x * 2.0 ** 50
    elif name == "nonfinite":
        nan, inf = float("nan"), float("inf")
        for i, row in enumerate(bad_ln_rows(rows)):
            c = [(11 * row + 3 + 64 * j) % d for j in range(3)]
            kind = i % 4
            if kind == 0:
                x[row, c[0]] = nan
            elif kind == 1:
                x[row, c[0]] = inf
            elif kind == 2:
                x[row, c[0]] = -inf
            else:
                x[row, c[0]], x[row, (c[0] + 1) % d], x[row, (c[0] + 2) % d] = nan, inf, -inf
    return _bf16(x)


def ln_weights(d, planted=True, seed=0):
    """(w, b), float32 holding bf16-representable values"""
    if not planted:
        return torch.ones(d), torch.zeros(d)
    g = _gen("lnw", d, seed)
    return _bf16(1.0 + 0.5 * torch.randn(d, generator=g)), _bf16(torch.randn(d, generator=g))


# ---------------------------------------------------------------------------------------------------- LayerNorm: reference, checker
def ln_reference(x, w, b, eps=LN_EPS):
    """float64 of layer_norm.py:88-93 on x [..., d]: {"scale" [...], "y" [..., d], "A" [..., d], "ratio" |mean| / scale [...]}"""
    x, w, b = x.double(), w.double(), b.double()
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    scale = (xc.pow(2).mean(-1, keepdim=True) + eps).sqrt()
    xn = xc / scale
    amp = 1.0 + mean.abs() / scale
    return {"scale": scale[..., 0], "y": xn * w + b, "A": (xn * w).abs() + b.abs() + w.abs() * amp, "ratio": (mean.abs() / scale)[..., 0]}


def ln_torch(x, w, b, eps=LN_EPS):
    """(scale, y) of layer_norm.py:88-93 in torch fp32: the bad rows' expectation, and the figure printed beside the kernel's"""
    x, w, b = x.float(), w.float(), b.float()
    x = x - x.mean(-1, keepdim=True)
    scale = (x.pow(2).mean(-1, keepdim=True) + eps).sqrt()
    return scale[..., 0], x / scale * w + b


def _ratio(err, bound):
    """worst err / bound; inf where no finite ratio satisfies the comparison (NaN errors included)"""
    r = err / bound
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    r = torch.where((err == 0) & (bound >= 0), torch.zeros_like(r), r)
    return float(r.max()) if r.numel() else 0.0


def _same_nonfinite(got, want):
    """got carries want's non-finite values: NaN where NaN, +-inf with the sign"""
    return bool(((torch.isnan(want) & torch.isnan(got)) | (got == want))[~torch.isfinite(want)].all())


def check_ln(x, w, b, scale=None, y32=None, y16=None, eps=LN_EPS):
    """{"scale" | "y32" | "y16": worst error / bound} of a LayerNorm of x [..., d]: ``scale`` [...] the fp32 hook_scale, ``y32`` an fp32
    hook_normalized / fp32 output, ``y16`` the bf16 output; each only when given.  Rows of x that hold a non-finite value must come back
    as torch fp32 of the reference's formula leaves them (NaN), every other row within the module docstring's bounds."""
    ref = ln_reference(x, w, b, eps)
    good = torch.isfinite(x).all(-1)
    t_scale, t_y = ln_torch(x, w, b, eps)
    out = {}

    def one(got, want, want_bad, bound):
        got = got.double().reshape(want.shape)
        r = _ratio((got - want).abs()[good], bound[good])
        return r if _same_nonfinite(got[~good], want_bad.double().reshape(want.shape)[~good]) else float("inf")

    if scale is not None:
        out["scale"] = one(scale, ref["scale"], t_scale, LN_FACTOR * U * ref["scale"])
    if y32 is not None:
        out["y32"] = one(y32, ref["y"], t_y, LN_FACTOR * U * ref["A"])
    if y16 is not None:
        out["y16"] = one(y16, ref["y"], t_y, BF16_EPS * ref["y"].abs() + LN_FACTOR * U * ref["A"])
    return out


def passes(ratios):
    return all(r <= 1.0 for r in ratios.values())


def report(tag, ratios, beside=None):
    line = f"{tag}: error / bound  " + "  ".join(f"{k} {v:.3g}" for k, v in ratios.items())
    if beside:
        line += "  (torch fp32 of the reference's formula, rounded to the storage dtype: " + "  ".join(f"{k} {v:.3g}" for k, v in beside.items()) + ")"
    return line


def ln_torch_ratios(x, w, b, bf16, eps=LN_EPS):
    """the same figures for torch fp32 of the reference's formula, its output rounded to the storage dtype"""
    s, y = ln_torch(x, w, b, eps)
    return check_ln(x, w, b, scale=s, y32=y, y16=y.to(torch.bfloat16) if bf16 else None, eps=eps)


# -------------------------------------------------------------------------------------------------------------- LayerNorm: CPU twin
LN_BUGS = ("one_pass", "no_eps", "eps_after_sqrt", "divisor_512", "skip_chunks_sum", "skip_chunks_write", "wb_chunk0",
           "last_row_unwritten", "nan_neighbours", "centred_in_bf16", "tap_from_bf16")


def _f32(a):
    return np.asarray(a, dtype=np.float32)


def _fma(a, b, c):
    """round(a b + c) for float32 operands (the product is exact in float64)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _wave_sum(v):
    """wave_sum of csrc/pv_common.hpp over the last axis (64 lanes): v += shfl_xor(v, o) for o = 32 .. 1"""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., lane ^ o]).astype(np.float32)
    return v[..., 0]


def ln_twin(x, w, b, eps=LN_EPS, fma=True, bug=None):
    """float32 twin of ln_kernel (csrc/rowops.hip) on x [rows, d] with the kernel's order of operations: lane L holds the 8-element
    chunks L, L + 64, L + 128, L + 192 and adds them up in that order, the 64 partial sums meet in the xor tree, mean and variance are
    true divisions by d, y = (x / scale) w + b.  ``fma``: the compiler's contraction of x x + sq and of (x / scale) w + b.
    Returns (scale [rows], y fp32 [rows, d], y rounded to bf16 [rows, d]); ``bug``: one of LN_BUGS, a twin that is wrong on purpose --
    where such a twin does not store, the value stays UNWRITTEN."""
    assert bug is None or bug in LN_BUGS
    with np.errstate(all="ignore"):
        x = _f32(x.numpy() if isinstance(x, torch.Tensor) else x)
        w = _f32(w.numpy() if isinstance(w, torch.Tensor) else w)
        b = _f32(b.numpy() if isinstance(b, torch.Tensor) else b)
        rows, d = x.shape
        nchunks = d // 8
        # [rows, lane, c, i] with zeros where lane + 64 c >= nchunks (the kernel skips them; adding 0 changes no sum)
        pad = np.zeros((rows, 2048), np.float32)
        pad[:, :d] = x
        xl = pad.reshape(rows, 4, 64, 8).transpose(0, 2, 1, 3).copy()
        live = (np.arange(64)[:, None] + 64 * np.arange(4)[None, :]) < nchunks                  # [lane, c]
        summed = live & (np.arange(4)[None, :] == 0) if bug == "skip_chunks_sum" else live
        n = np.float32(512 * math.ceil(d / 512) if bug == "divisor_512" else d)

        def lanes(v):                                     # per lane: sequential over c, then i
            acc = np.zeros((rows, 64), np.float32)
            for c in range(4):
                for i in range(8):
                    acc = (acc + np.where(summed[None, :, c], v[:, :, c, i], np.float32(0))).astype(np.float32)
            return acc

        mean = (_wave_sum(lanes(xl)) / n).astype(np.float32)
        if bug == "one_pass":
            sq = np.zeros((rows, 64), np.float32)
            for c in range(4):
                for i in range(8):
                    t = np.where(summed[None, :, c], xl[:, :, c, i], np.float32(0))
                    sq = _fma(t, t, sq)
            var = ((_wave_sum(sq) / n).astype(np.float32) - mean * mean).astype(np.float32)
            xc = (xl - mean[:, None, None, None]).astype(np.float32)
        else:
            xc = (xl - mean[:, None, None, None]).astype(np.float32)
            if bug == "centred_in_bf16":
                xc = torch.from_numpy(xc).to(torch.bfloat16).float().numpy()
            sq = np.zeros((rows, 64), np.float32)
            for c in range(4):
                for i in range(8):
                    t = np.where(summed[None, :, c], xc[:, :, c, i], np.float32(0))
                    sq = _fma(t, t, sq) if fma else (sq + (t * t).astype(np.float32)).astype(np.float32)
            var = (_wave_sum(sq) / n).astype(np.float32)
        e = np.float32(eps)
        if bug == "no_eps":
            scale = np.sqrt(var).astype(np.float32)
        elif bug == "eps_after_sqrt":
            scale = (np.sqrt(var).astype(np.float32) + e).astype(np.float32)
        else:
            scale = np.sqrt((var + e).astype(np.float32)).astype(np.float32)
        wl = np.zeros(2048, np.float32)
        bl = np.zeros(2048, np.float32)
        wl[:d], bl[:d] = w, b
        wl = wl.reshape(4, 64, 8).transpose(1, 0, 2)
        bl = bl.reshape(4, 64, 8).transpose(1, 0, 2)
        if bug == "wb_chunk0":
            wl, bl = np.repeat(wl[:, :1], 4, axis=1), np.repeat(bl[:, :1], 4, axis=1)
        q = (xc / scale[:, None, None, None]).astype(np.float32)
        y = _fma(q, np.broadcast_to(wl, q.shape), np.broadcast_to(bl, q.shape)) if fma else ((q * wl).astype(np.float32) + bl).astype(np.float32)
        if bug == "skip_chunks_write":
            y[:, :, 1:, :] = UNWRITTEN
        y = y.transpose(0, 2, 1, 3).reshape(rows, 2048)[:, :d].copy()
        if bug == "last_row_unwritten":
            y[3::4] = UNWRITTEN
            scale[3::4] = UNWRITTEN
        if bug == "nan_neighbours":
            bad = ~np.isfinite(x).all(-1)
            for g0 in range(0, rows, 4):
                if bad[g0:g0 + 4].any():
                    y[g0:g0 + 4] = np.nan
                    scale[g0:g0 + 4] = np.nan
    y_t = torch.from_numpy(y)
    y16 = y_t.to(torch.bfloat16)
    if bug == "tap_from_bf16":
        y_t = y16.float()
    return torch.from_numpy(scale), y_t, y16


# ------------------------------------------------------------------------------------------------------------ activation: inputs
def all_bf16():
    """the 65 536 bf16 bit patterns in order, as a bfloat16 tensor"""
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)


def finite_bf16():
    """the 65 280 finite ones"""
    a = all_bf16()
    return a[torch.isfinite(a.float())]


def fp32_extra(n, seed=0):
    """n fp32 values that are not bf16-exact: uniform in bit pattern over |x| < 2^7 (denormals included), the last 4096 uniform in
    [-9, -3]"""
    assert n > 8192
    g = _gen("fp32_extra", n, seed)
    m = n - 4096
    bits = torch.randint(0, (127 + 7) << 23, (m,), generator=g, dtype=torch.int64)
    bits = bits | torch.where((bits & 0xFFFF) == 0, 1, 0)                                      # never bf16-exact
    bits = bits | (torch.randint(0, 2, (m,), generator=g, dtype=torch.int64) << 31)
    a = torch.from_numpy(bits.numpy().astype(np.uint32).view(np.float32).copy())
    tail = -9.0 + 6.0 * torch.rand(4096, generator=g, dtype=torch.float64)
    tail = tail.float()
    tail = torch.where(_bf16(tail) == tail, tail + 2.0 ** -20, tail)
    return torch.cat([a, tail])


# ---------------------------------------------------------------------------------------------- activation: reference, checker
def act_reference(act, x):
    """float64, accurate in the negative tail, of x as stored"""
    x = x.double()
    if act == "gelu":
        return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))
    if act == "quick_gelu":
        return x / (1.0 + torch.exp(-1.702 * x))
    assert act == "relu"
    return torch.clamp_min(x, 0.0)


def act_torch(act, x):
    """the reference's own functions in torch fp32 (mlp.py:41-63: F.gelu, activation_fns.quick_gelu, F.relu)"""
    x = x.float()
    if act == "gelu":
        return torch.nn.functional.gelu(x)
    if act == "quick_gelu":
        return x * torch.sigmoid(1.702 * x)
    return torch.relu(x)


def act_formula(act, x):
    """the reference's formulas written out in torch fp32: the expectation for non-finite inputs"""
    x = x.float()
    if act == "gelu":
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    return act_torch(act, x)


def act_bound(act, bf16, x, ref):
    x, ref = x.double().abs(), ref.abs()
    floor = 2.0 ** -23 * x + 2.0 ** -126
    if bf16:
        return BF16_EPS * ref + floor
    if act == "quick_gelu":
        return (2.0 ** -21 + 2.0 ** -23 * 1.702 * x) * ref + floor
    return 2.0 ** -21 * ref + GELU_FP32_TAIL * x + 2.0 ** -126


def check_act(act, bf16, x, got):
    """{"post": worst error / bound} of got = act(x) stored in bf16 / fp32; x of any shape, non-finite values allowed (see the module
    docstring for what they must give)."""
    x, got = x.reshape(-1).double(), got.reshape(-1).double()
    fin = torch.isfinite(x)
    want = act_formula(act, x[~fin]).double()                                                     # NaN, +inf, or relu(-inf) = 0
    ok = _same_nonfinite(got[~fin], want) and bool((got[~fin] == want)[torch.isfinite(want)].all())
    xf, gf = x[fin], got[fin]
    ref = act_reference(act, xf)
    if act == "relu":
        r = 0.0 if bool((gf == ref).all()) else float("inf")
    else:
        r = _ratio((gf - ref).abs(), act_bound(act, bf16, xf, ref))
    return {"post": r if ok else float("inf")}


def act_torch_ratio(act, bf16, x):
    """the same figure for torch fp32 of the reference's formula, rounded to the storage dtype"""
    y = act_torch(act, x)
    return check_act(act, bf16, x, y.to(torch.bfloat16) if bf16 else y)


# ----------------------------------------------------------------------------------------------------------- activation: CPU twins
ACT_BUGS = ("tanh_gelu", "swapped", "c17", "zero_tail", "identity_head")


def _exp2(t, flush):
    with np.errstate(all="ignore"):
        e = np.exp2(t.astype(np.float64)).astype(np.float32)
    return np.where(np.abs(e) < np.float32(2.0 ** -126), np.float32(0), e) if flush else e


def _rcp(t, flush):
    with np.errstate(all="ignore"):
        r = (1.0 / t.astype(np.float64)).astype(np.float32)
    return np.where(np.abs(r) < np.float32(2.0 ** -126), np.float32(0), r) if flush else r


def act_twin(act, x, bug=None, flush=False):
    """float32 twin of act2<ACT> (csrc/gemm_epi.hpp) with an exact exp2 and reciprocal in place of v_exp_f32 / v_rcp_f32; ``flush``: both
    return 0 for a denormal result, as the hardware instructions may.  x: a float32 tensor; returns float32 (unrounded).  ``bug``: one
    of ACT_BUGS, a twin that is wrong on purpose."""
    assert bug is None or bug in ACT_BUGS
    if bug == "swapped":
        return act_twin({"gelu": "quick_gelu", "quick_gelu": "gelu"}[act], x, None, flush)
    one = np.float32(1.0)
    with np.errstate(all="ignore"):
        xv = _f32(x.numpy())
        if bug == "tanh_gelu":
            x3 = (xv * xv * xv).astype(np.float32)
            inner = (np.float32(math.sqrt(2.0 / math.pi)) * (xv + np.float32(0.044715) * x3)).astype(np.float32)
            y = (np.float32(0.5) * xv * (one + np.tanh(inner).astype(np.float32))).astype(np.float32)
        elif act == "quick_gelu":
            k = np.float32(np.float32(-1.7 if bug == "c17" else -1.702) * np.float32(1.4426950408889634))
            t = (xv * k).astype(np.float32)
            dd = (_exp2(t, flush) + one).astype(np.float32)
            y = (xv * _rcp(dd, flush)).astype(np.float32)
        elif act == "gelu":
            z = (xv * np.float32(0.70710678118654752440)).astype(np.float32)
            az = np.abs(z)
            den = _fma(az, np.full_like(az, 0.3275911), np.full_like(az, 1.0))
            t = _rcp(den, flush)
            q = _fma(t, np.full_like(t, 1.061405429), np.full_like(t, -1.453152027))
            q = _fma(t, q, np.full_like(t, 1.421413741))
            q = _fma(t, q, np.full_like(t, -0.284496736))
            q = _fma(t, q, np.full_like(t, 0.254829592))
            q = (q * t).astype(np.float32)
            a2 = ((az * az).astype(np.float32) * np.float32(-1.4426950408889634)).astype(np.float32)
            e = _exp2(a2, flush)
            r = _fma(-q, e, np.full_like(q, 1.0))
            r = np.copysign(r, z)
            hx = (xv * np.float32(0.5)).astype(np.float32)
            y = _fma(hx, r, hx)
        else:
            y = np.maximum(xv, np.float32(0))
        if bug == "zero_tail":
            y = np.where(xv < -3, np.float32(0), y)
        if bug == "identity_head":
            y = np.where(xv > 3, xv, y)
    return torch.from_numpy(y)


# ------------------------------------------------------------------------------------------------- token mean and L2 normalise
def check_token_mean(x, got, t0, bf16):
    """worst error / bound of got [B, d] = mean over tokens t0 .. T - 1 of x [B, T, d], per column: fp32 2^-21 mean_t |x|; bf16
    2^-8 |ref| + 2^-21 mean_t |x| (one rounding of an fp32-accumulated mean whose partial sums never exceed sum_t |x|)"""
    x, got = x.double()[:, t0:], got.double()
    ref, mag = x.mean(1), x.abs().mean(1)
    return _ratio((got - ref).abs(), (BF16_EPS * ref.abs() if bf16 else 0.0) + 2.0 ** -21 * mag + 1e-300)


def l2norm_units(n):
    """the bound of an fp32 x / max(||x||, 1e-12) over n elements in units of u = 2^-24, relative to each element: the sum of n squares
    (each rounded once; all terms positive, so every addition costs at most u of the final sum) goes through at most
    ceil(n / 64) additions per lane and 6 in the xor tree, the square root halves that relative error and adds its own u, the division
    adds one more"""
    return (math.ceil(n / 64) + 6 + 1) / 2.0 + 2.0


def check_l2norm(x, got, bf16):
    """worst error / bound of got [rows, n] against float64 x / max(||x||, 1e-12), per element: fp32 l2norm_units(n) u |ref|, bf16
    2^-8 |ref| more; an all-zero row must stay zero"""
    x, got = x.double(), got.double()
    ref = x / x.pow(2).sum(-1, keepdim=True).sqrt().clamp_min(1e-12)
    bound = (l2norm_units(x.shape[-1]) * U + (BF16_EPS if bf16 else 0.0)) * ref.abs()
    return _ratio((got - ref).abs(), bound)
