"""Planted inputs for pv_logit_lens (csrc/lens.hip), their float64 truth and the per-element bound.  No GPU needed here.

A case is S taps [N, d] (bf16-representable, distinct per stack entry), answers [O, d] (bf16-representable, mean offset 0.02 so
that their row sums are not zero) and scale [N] = sqrt(var + 1e-5) of the LAST entry's rows in float64, rounded to fp32 -- what
ln_final caches.

Rows:  0 plain Gaussian | 1 three outlier channels at 30 x | 2 shifted by +100 (the mean term dominates) | 3 constant (its
centred value is zero) | 4 one NaN | 5 one +inf | from 6 on, by n % 3, pushed along an answer direction so that the top form has
known results: 0 a winner column w(n); 1 column 3 -- and column 259, whose answer row is a copy of row 3 and sits in the second
N-tile, so the expected index is 3; 2 the label column 7 -- its copies 5 (equal, lower index: counted) and 260 (equal, higher: not
counted) and column 9 = 1.5 x row 7 (above: counted), so top = 9 and rank = 2.

Truth: ((x - mean x) . a) / scale in float64.  Bound for any fp32 summation order of the algebraic form:
    |got - truth| <= (d + 4) 2^-24 (sum_k |x_k a_k| + |mean| sum_k |a_k|) / scale
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

U24 = 2.0 ** -24
LABEL, LABEL_LOW, LABEL_HIGH, LABEL_ABOVE = 7, 5, 260, 9
TIE_LOW, TIE_HIGH = 3, 259
FIRST_FREE = 10                       # winner columns are drawn from [FIRST_FREE, O) minus the planted ones
BOOST_768 = 40.0                      # times sqrt(768 / d): the cached scale grows with the push, so narrow rows need a harder one
SPECIAL_ROWS = 6

SHAPES = [(N, S, O, d) for N in (34, 260) for S in (1, 5) for O in (24, 264) for d in (64, 96, 768)]
# beyond the grid: a width whose last 64-byte K slab is ragged (d * 2 = 144 bytes: the chunk mask of the K-tail form)
SHAPES.append((34, 5, 264, 72))


def shape_id(shape) -> str:
    return "N{}-S{}-O{}-d{}".format(*shape)


def bf16(a: np.ndarray) -> np.ndarray:
    """round to bf16 (nearest even), back as float32"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy()


@dataclass
class Case:
    N: int
    S: int
    O: int
    d: int
    taps: np.ndarray            # [S, N, d] float32, bf16-representable
    answers: np.ndarray         # [O, d]
    scale: np.ndarray           # [N] float32
    truth: np.ndarray           # [N, S, O] float64 (NaN in the rows 4, 5)
    bound: np.ndarray           # [N, S, O] float64
    finite: np.ndarray          # [N] bool
    want_top: np.ndarray        # [N] int: the planted top column, -1 where none is planted
    want_rank: np.ndarray       # [N] int: the planted rank of LABEL, -1 where none is planted


def winner_column(n: int, O: int) -> int:
    free = [c for c in range(FIRST_FREE, O) if c not in (TIE_HIGH, LABEL_HIGH)]
    return free[(13 * n) % len(free)]


@functools.lru_cache(maxsize=None)
def make_case(N: int, S: int, O: int, d: int, seed: int = 0) -> Case:
    assert N > SPECIAL_ROWS + 3 and O > FIRST_FREE + 2
    rng = np.random.default_rng(1000 * seed + 7 * N + 11 * S + 13 * O + d)
    a = 0.05 * rng.standard_normal((O, d)) + 0.02
    a = bf16(a)
    a[LABEL_LOW] = a[LABEL]
    a[LABEL_ABOVE] = bf16(1.5 * a[LABEL])
    if O > LABEL_HIGH:
        a[TIE_HIGH] = a[TIE_LOW]
        a[LABEL_HIGH] = a[LABEL]
    x = rng.standard_normal((S, N, d)) * (1.0 + 0.25 * np.arange(S))[:, None, None]
    x[:, 1, [1, d // 2, d - 3]] *= 30.0
    x[:, 2] += 100.0
    x[:, 3] = (1.5 + 0.5 * np.arange(S))[:, None]
    want_top = np.full(N, -1)
    want_rank = np.full(N, -1)
    for n in range(SPECIAL_ROWS, N):
        col = (winner_column(n, O), TIE_LOW, LABEL)[n % 3]
        x[:, n] += BOOST_768 * np.sqrt(768.0 / d) * a[col]
        want_top[n] = (col, TIE_LOW, LABEL_ABOVE)[n % 3]
        if n % 3 == 2:
            want_rank[n] = 2
    x = bf16(x)
    x[:, 4, d // 3] = np.nan
    x[:, 5, d // 5] = np.inf
    finite = np.ones(N, bool)
    finite[[4, 5]] = False

    x64, a64 = x.astype(np.float64), a.astype(np.float64)
    with np.errstate(invalid="ignore"):
        mean = x64.mean(axis=-1)                                               # [S, N]
        xc = x64 - mean[..., None]
        scale = np.sqrt((xc[-1] ** 2).mean(axis=-1) + 1e-5).astype(np.float32)   # [N]; NaN in the rows 4, 5
        sc = scale.astype(np.float64)[None, :, None]
        truth = (xc @ a64.T) / sc                                              # [S, N, O]
        bound = (d + 4) * U24 * (np.abs(x64) @ np.abs(a64).T + np.abs(mean)[..., None] * np.abs(a64).sum(-1)) / sc
    truth, bound = truth.transpose(1, 0, 2), bound.transpose(1, 0, 2)
    assert np.isnan(truth[~finite]).all() and np.isfinite(truth[finite]).all()

    # the planted results hold in the truth with a margin above twice the bound
    for n in range(SPECIAL_ROWS, N):
        for s in range(S):
            t, b = truth[n, s], bound[n, s]
            w = want_top[n]
            same = [w] + ([TIE_HIGH] if (w == TIE_LOW and O > TIE_HIGH) else [])
            others = np.delete(np.arange(O), same)
            assert (t[w] - t[others] > 2 * (b[w] + b[others])).all(), (n, s, "winner margin")
            if want_rank[n] >= 0:
                equal = [c for c in (LABEL, LABEL_LOW, LABEL_HIGH) if c < O]
                assert all(t[c] == t[LABEL] for c in equal)
                below = np.delete(np.arange(O), equal + [LABEL_ABOVE])
                assert (t[LABEL] - t[below] > 2 * (b[LABEL] + b[below])).all(), (n, s, "label margin")
                assert t[LABEL_ABOVE] - t[LABEL] > 2 * (b[LABEL_ABOVE] + b[LABEL])
    return Case(N, S, O, d, x, a, scale, truth, bound, finite, want_top, want_rank)


def reference_bf16_centring(case: Case) -> np.ndarray:
    """What the reference's own bf16 path computes (mean and centred rows rounded to bf16, the rest in fp32), as float64
    [N, S, O]: the form a kernel must NOT take -- it sits far outside the bound."""
    x = torch.from_numpy(case.taps).to(torch.bfloat16)
    xc = x - x.mean(dim=-1, keepdim=True)
    out = (xc.float() / torch.from_numpy(case.scale)[None, :, None]).double() @ torch.from_numpy(case.answers).double().T
    return out.permute(1, 0, 2).numpy()


def top_of(directions: np.ndarray, label: Optional[int]):
    """(top_idx, rank) of directions [..., O] by the package's rule: lowest index among the largest; larger logits plus equal
    ones at a lower index; NaN rows: index 0, rank -1"""
    nan_row = np.isnan(directions).any(axis=-1)
    safe = np.where(np.isnan(directions), -np.inf, directions)
    idx = np.where(nan_row, 0, safe.argmax(axis=-1))
    rank = None
    if label is not None:
        lab = safe[..., label:label + 1]
        lower = np.arange(directions.shape[-1]) < label
        rank = ((safe > lab) | ((safe == lab) & lower)).sum(axis=-1)
        rank = np.where(nan_row, -1, rank)
    return idx, rank
