"""Adversarial q, k, v for the attention kernels, their float64 reference and the bound checker (plain torch, any device).

The GPU suite otherwise feeds the kernels what a randomly initialised ViT produces: scores within +-0.4 of zero, rows whose spread
stays under 0.8, pattern elements under 2^-8.  On such inputs an absolute 2^-8 pattern bound accepts an all-zero pattern, and an
online softmax whose rescale is dropped hides under the rounding.  The cases here are built so that it cannot:

``peaked``     k[..., 0] follows a profile over the key index, one per (image, head):
                 (0, 0) an ascending ramp -- the running maximum rises in every 32-key tile and ends on key T - 1 in the ragged last tile
                 (0, 1) a descending ramp -- the maximum is key 0
                        (both 0.875 rank / T with the end key alone at 1: the top of a plain ramp would tie after rounding to bf16)
                 (1, 0) equal spikes at keys 0, 31, 32, 63, 64, T - 2, T - 1 (both sides of the first two tile edges, the last
                        tile); components 1..7 of k name the spikes, and the query picks through them which one is the row's maximum
                 (1, 1) a plateau of eight equal maxima across the edge between keys 31 and 32
               q[..., 0] cycles per query over the gains {0, 4, 16, 64} sqrt(d_head): near-uniform to one-hot rows inside every group of
               32 consecutive queries (one wave).  Row spread <= 64 + 8 = 72.
``shifted``    the same geometry at gains {0, 0.5, 2, 8} (spread <= 9) plus a common offset per row through the last component
               (q = +-1000, k = sqrt(d_head)): about +1000 on even rows, -1000 on odd rows, |s| < 1024.  A pad key scored 0 swallows
               an odd row; exp(s) without the max overflows on an even one.
``nonfinite``  the ``shifted`` geometry without the offset (profiles moved off zero so that inf * 0 never arises in a real key), then
                 (0, 0) query 5 all NaN; query 40 (9 when T <= 64) +inf in component 0 against k[..., 0] > 0: every score +inf;
                        query T - 1 (the last partial 128-query block) -inf there: every score -inf
                 (1, 0) query T - 1 +inf against a k[..., 0] of both signs: +inf and -inf mixed
                 (1, 1) key T / 2 all NaN: every row of that head is bad
               Image 0, head 1 has no bad row; queries 5 and 40 (9) of (0, 0) sit among the good rows of their group of 32.
``benign``     noise only: what the older tests feed.  Not a GPU case -- it shows what the older absolute bound accepts.

All values are exactly representable in bf16 (built in fp32, rounded to bf16, returned as fp32), so one set serves both dtypes and the
reference starts from the same numbers as the kernel.

Bounds (``check``), with eps = 2^-8 for bf16 and FP32_TOL = 1e-4 for fp32:
  scores   against q k / attn_scale in float64.  bf16: per row |got - ref| <= eps max_row|ref| + 1e-6 (one rounding of an fp32 sum);
           fp32: relative L2 of the row < FP32_TOL.  Non-finite positions must match exactly (NaN where NaN, +-inf with the sign).
  pattern  against the float64 softmax of the STORED scores, NaN -> 0 (as the reference model computes it).  bf16: per ELEMENT
           |got - ref| <= eps ref + 1e-30 -- one rounding to bf16 (8 significant bits: half an ulp is at most 2^-8 / (1 + 2^-8) =
           0.996 eps of the value, reached just above a power of two; 2^-9 on average) plus the fp32 exp and sum error before it (a
           kernel that forms s log2e - m log2e in fp32 loses about 1024 * 2^-22 = 2.4e-4 relative at |s| = 1024, T <= 2048, which
           counts only where it turns the rounding); below 1e-30 the kernel may flush.  No element is excluded.  What the rounding
           alone costs on a given input is what a float32 torch softmax of the same stored scores, rounded to bf16, scores against
           the same bound: the GPU test prints it next to the kernel's (MEASURED.md: equal to three digits on every path).
           fp32: relative L2 of each row < FP32_TOL.
  z        against (stored pattern) v in float64, per (image, query, head) row: bf16 eps max_row|ref| + 1e-6, fp32 relative L2.
  Rows the reference zeroes must be exactly zero in pattern and z.
``check`` returns the worst error / bound ratio per quantity (inf for a mismatch that has no bound: a misplaced non-finite value, a
non-zero in a zeroed row); bf16 passes at ratio <= 1, fp32 at ratio < 1 (``passes``).
"""
import math

import torch

FP32_TOL = 1e-4
BF16_EPS = 2.0 ** -8
CASES = ("peaked", "shifted", "nonfinite")
B, H = 2, 2
SPIKE_KEYS = (0, 31, 32, 63, 64, -2, -1)
GAINS = (0.0, 4.0, 16.0, 64.0)


def _bf16(t):
    return t.to(torch.bfloat16).to(torch.float32)


def spike_keys(T):
    """the spike positions that exist at T, in SPIKE_KEYS order, each once"""
    out = []
    for j in SPIKE_KEYS:
        j = j + T if j < 0 else j
        if 0 <= j < T and j not in out:
            out.append(j)
    return out


def plateau_keys(T):
    lo = 28 if T >= 36 else max(T // 2 - 4, 0)
    return list(range(lo, min(lo + 8, T)))


def bad_rows(T):
    """nonfinite: {(image, head): query rows that must come back as zeros} ((1, 1): all of them)"""
    return {(0, 0): sorted({5, 40 if T > 64 else 9, T - 1}), (0, 1): [], (1, 0): [T - 1], (1, 1): list(range(T))}


def make_case(name, T, dh, seed=0):
    """(q, k, v), each [B, T, H, dh] float32 on the CPU holding bf16-representable values"""
    assert name in CASES + ("benign",) and T >= 17 and dh >= 16
    g = torch.Generator().manual_seed(1000 * seed + 7 * T + dh)
    q, k, v = (0.1 * torch.randn(B, T, H, dh, generator=g) for _ in range(3))
    if name == "benign":
        return _bf16(q), _bf16(k), _bf16(v)
    root = math.sqrt(dh)
    j = torch.arange(T, dtype=torch.float32)
    spikes, plateau = spike_keys(T), plateau_keys(T)
    prof = torch.zeros(B, H, T)
    # ramps: 0.875 (rank / T), the end key alone at 1 -- bf16 holds 128 values per binade, so a plain ramp would tie at its top
    prof[0, 0] = 0.875 * (j + 1) / T
    prof[0, 0, T - 1] = 1.0
    prof[0, 1] = 0.875 * (T - j) / T
    prof[0, 1, 0] = 1.0
    prof[1, 0, spikes] = 1.0
    prof[1, 1, plateau] = 1.0
    if name == "nonfinite":
        prof[1] -= 0.25                              # spikes / plateau: {-0.25, 0.75}: both signs, never 0
    k[..., 0] = prof.permute(0, 2, 1)
    k[1, :, 0, 1:1 + len(SPIKE_KEYS)] = 0.0
    for i, key in enumerate(spikes):
        k[1, key, 0, 1 + i] = 1.0                    # component 1 + i names spike i
    r = torch.arange(T)
    gain = torch.tensor(GAINS)[r % 4] * (1.0 if name == "peaked" else 0.125)
    q[..., 0] = (gain * root)[None, :, None]
    # (1, 0): query r lifts spike (r // 4) mod n by gain / 8 over the others -- the row's maximum walks over the spikes
    q[1, :, 0, 1:1 + len(SPIKE_KEYS)] = 0.0
    q[1, r, 0, 1 + (r // 4) % len(spikes)] = gain * root / 8
    if name == "shifted":
        q[..., dh - 1] = torch.where(r % 2 == 0, 1000.0, -1000.0)[None, :, None]
        k[..., dh - 1] = root
    if name == "nonfinite":
        nan_q, pinf_q, ninf_q = bad_rows(T)[(0, 0)]
        q[0, nan_q, 0, :] = float("nan")
        q[0, pinf_q, 0, 0] = float("inf")
        q[0, ninf_q, 0, 0] = float("-inf")
        q[1, T - 1, 0, 1:1 + len(SPIKE_KEYS)] = 0.0  # (finite times the spike names; the +inf goes into component 0 alone)
        q[1, T - 1, 0, 0] = float("inf")
        k[1, T // 2, 1, :] = float("nan")
    return _bf16(q), _bf16(k), _bf16(v)


def reference_scores(q, k, dh):
    """q k / attn_scale in float64, [B, H, T, T]"""
    return torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) / math.sqrt(dh)


def reference_pattern(s_stored):
    """float64 softmax of the stored scores, NaN -> 0 (attention.py:148-150)"""
    p = torch.softmax(s_stored.double(), dim=-1)
    return torch.where(torch.isnan(p), torch.zeros_like(p), p)


def _ratio(err, bound):
    """worst err / bound; inf where the comparison is not satisfied by any finite ratio (NaN errors included)"""
    r = err / bound
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max()) if r.numel() else 0.0


def _rel_l2_rows(got, ref, dim=-1):
    den = ref.pow(2).sum(dim).sqrt().clamp_min(1e-300)
    return (got - ref).pow(2).sum(dim).sqrt() / den


def check(dtype, q, k, v, s_got, p_got, z_got, dh):
    """{"scores" | "pattern" | "z": worst error / bound} of the taps s_got, p_got [B, H, T, T] and z_got [B, T, H, dh] of a kernel run
    on q, k, v in `dtype` (torch.bfloat16 / torch.float32); see the module docstring for the bounds."""
    bf16 = dtype == torch.bfloat16
    s_got, p_got, z_got = s_got.double(), p_got.double(), z_got.double()
    out = {}
    inf = float("inf")

    # scores
    s_ref = reference_scores(q, k, dh)
    fin = torch.isfinite(s_ref)
    same_nonfinite = torch.where(fin, torch.isfinite(s_got), (torch.isnan(s_ref) & torch.isnan(s_got)) | (s_got == s_ref))
    ref0, got0 = torch.where(fin, s_ref, torch.zeros_like(s_ref)), torch.where(fin & torch.isfinite(s_got), s_got, torch.zeros_like(s_got))
    if bf16:
        bound = BF16_EPS * ref0.abs().amax(-1, keepdim=True) + 1e-6
        r = _ratio((got0 - ref0).abs(), bound.expand_as(ref0))
    else:
        r = _ratio(_rel_l2_rows(got0, ref0), torch.full(ref0.shape[:-1], FP32_TOL, dtype=torch.float64, device=ref0.device))
    out["scores"] = r if bool(same_nonfinite.all()) else inf

    # pattern, against the softmax of the stored scores
    p_ref = reference_pattern(s_got)
    zeroed = p_ref.amax(-1) == 0                                   # [B, H, T]: rows the reference zeroes
    if bf16:
        r = _ratio((p_got - p_ref).abs(), BF16_EPS * p_ref + 1e-30)
    else:
        live = ~zeroed
        r = _ratio(_rel_l2_rows(p_got, p_ref)[live], torch.full((int(live.sum()),), FP32_TOL, dtype=torch.float64, device=p_ref.device))
    if bool((p_got[zeroed] != 0).any()):
        r = inf
    out["pattern"] = r

    # z, against the stored pattern times v
    z_ref = torch.einsum("bhqk,bkhd->bqhd", p_got, v.double())
    if bf16:
        bound = BF16_EPS * z_ref.abs().amax(-1, keepdim=True) + 1e-6
        r = _ratio((z_got - z_ref).abs(), bound.expand_as(z_ref))
    else:
        live = ~zeroed.permute(0, 2, 1)
        r = _ratio(_rel_l2_rows(z_got, z_ref)[live], torch.full((int(live.sum()),), FP32_TOL, dtype=torch.float64, device=z_ref.device))
    if bool((z_got[zeroed.permute(0, 2, 1)] != 0).any()):
        r = inf
    out["z"] = r
    return out


def passes(dtype, ratios):
    return all((r <= 1.0) if dtype == torch.bfloat16 else (r < 1.0) for r in ratios.values())


def report(tag, ratios):
    return f"{tag}: error / bound  " + "  ".join(f"{k} {v:.3g}" for k, v in ratios.items())


def pattern_elementwise_ok(p_got, p_ref):
    """the bf16 element bound alone (for the older tests, next to their absolute one): (ok, worst error / bound)"""
    r = _ratio((p_got.double() - p_ref.double()).abs(), BF16_EPS * p_ref.double() + 1e-30)
    return r <= 1.0, r
