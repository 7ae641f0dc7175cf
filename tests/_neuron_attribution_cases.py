"""Planted inputs for pv_neuron_attribution / pv_neuron_attribution_topk (csrc/attribution_neuron.hip), their float64 truth, the
per-element bound and the top-k oracle.  No GPU needed here.

A case is L taps post [B, T, M] and L matrices W_out [M, d] (both bf16-representable, distinct per layer), fp32 answers (NOT
bf16-representable: 0.05 x Gaussian + 0.02, the offset so that centring matters) and a positive fp32 scale [B, T].  Shared answers
are [O, d]; per-image answers are [B, O, d] with image 1's the exact negation of image 0's, and then image 1 also holds image 0's
post and scale, so that its outputs must be the exact negatives of image 0's -- which they are only if the kernel picks the
answers by the row's image.

Tokens (in every image):
  0 plain Gaussian | 1 three outlier neurons at 30 x in every layer | 2 one NaN neuron (layer 0) and one +inf neuron (the last
  layer): NaN in all their columns, every other neuron of the row finite; for the top-k the NaN entries come first, in index order
  3 the TIE token: four neurons with the same post (8) and the same W_out row -- two in layer 0 and two in layer 1 where L >= 2 --
    that row being the sum of the centred answers (image 0's when they are per image), so that the four values are bit-identical
    and the largest of the row in magnitude in every column, and the largest in value wherever the answers are not the negated
    ones (with answers per image: in images 0 and 1, and in image 0; a third image has answers of its own); k = 2 and k = 3 cut
    the tie
  4 the SPARSE token: every neuron zero except five, three of them positive and two negative in column 0 of image 0: any k > 5
    ends in a mass tie of +-0, above the top-k kernel's candidate capacity (1024) on the shapes with L M > 1024
  from 5 on plain.

Truth, float64:  out[b, t, l M + n, o] = post[l, b, t, n] (W_out[l, n] . (a_o - mean(a_o))) / scale[b, t]; where post is NaN or
an infinity the truth is NaN (the reference's mean over that neuron's d_model values is not finite).

Bound for the folded form  fl(fl(post G) / scale),  G_n = sum_k W_nk ac_k,  ac = a - mean(a)  (u = 2^-24), derived as for the heads
(tests/_attribution_cases.py):
  * ac^: |ac^_k - ac_k| <= (d + 2) u (|a_k| + mean|a|); G_n: d products and a sum of d terms in some order: relative (d + 1) u on
    sum_k |W_nk| |ac^_k|
  * one product post G and one division: u each
  together, to first order, with A_n = sum_k |W_nk| (|a_k| + mean_k |a_k|):
    |got - truth| <= ((d + 2) + (d + 1) + 1 + 1) u |post| A_n / scale <= (2 d + 8) u |post| A_n / scale
  The constant 2 d + 8 leaves 3 u for the second-order terms.  Derived, not measured.

The top-k oracle, topk_order(values, k, by): per (..., answer) the k flat indices with the largest key, key = value (by = 0) or
|value| (by = 1) compared as floats with -0 folded onto +0, NaN above everything, ties to the lowest index: a numpy lexsort on
(not NaN, -key, index).
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np
import torch

U24 = 2.0 ** -24
TOPK_CAP = 1024              # NATTR_CAP of csrc/attribution_neuron.hip: more candidates than this take the radix-select path
# (B, T, L, M, d, O)
SHAPES = [
    (3, 6, 2, 40, 96, 1),             # M below one fold tile, rows shorter than a row tile
    (2, 50, 3, 3072, 768, 4),         # the bench geometry
    (2, 7, 2, 1288, 320, 16),         # M no multiple of 64, at the answer cap
    (2, 197, 1, 2048, 256, 3),        # several row tiles per image
]
TOK_OUTLIER, TOK_NONFINITE, TOK_TIE, TOK_SPARSE = 1, 2, 3, 4
TIE_POST = 8.0


def shape_id(shape) -> str:
    return "B{}-T{}-L{}-M{}-d{}-O{}".format(*shape)


def bf16(a: np.ndarray) -> np.ndarray:
    """round to bf16 (nearest even), back as float32"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def tie_neurons(L: int, M: int):
    """the four (layer, neuron) of the TIE token, in flat-index order"""
    if L >= 2:
        return [(0, 3), (0, M - 2), (1, 5), (1, M // 2 + 1)]
    return [(0, 3), (0, 5), (0, M // 2 + 1), (0, M - 2)]


def sparse_neurons(L: int, M: int):
    """the five (layer, neuron, sign of the value in column 0 of image 0, |post|) of the SPARSE token"""
    return [(0, 2, +1, 3.0), (0, M - 7, -1, 2.75), (L - 1, M // 2, +1, 2.5), (L - 1, 9, -1, 2.25), (L // 2, M // 4 + 1, +1, 2.0)]


def nonfinite_neurons(L: int, M: int):
    """(layer, neuron) of the NaN and of the +inf of the NONFINITE token"""
    return (0, M // 3), (L - 1, M // 5)


@dataclass
class Case:
    shape: tuple
    per_image: bool
    post: np.ndarray            # [L, B, T, M] float32, bf16-representable (NaN / inf planted)
    W_out: np.ndarray           # [L, M, d] float32, bf16-representable
    answers: np.ndarray         # [O, d] or [B, O, d] float32
    scale: np.ndarray           # [B, T] float32, positive
    truth: np.ndarray           # [B, T, L * M, O] float64 (NaN in the planted neurons)
    bound: np.ndarray           # [B, T, L * M, O] float64
    nan: np.ndarray             # [B, T, L * M] bool: neurons that must be NaN in every column
    zero: np.ndarray            # [B, T, L * M] bool: neurons that must be exactly (+-) 0 in every column


def folded(W_out, answers, B):
    """(G, A) float64 [L, M, B, O]: G = W_out . (a - mean a), A = |W_out| . (|a| + mean|a|)"""
    a = answers.astype(np.float64)
    if a.ndim == 2:
        a = np.broadcast_to(a, (B, *a.shape))
    w = W_out.astype(np.float64)
    G = np.einsum("lnk,bok->lnbo", w, a - a.mean(axis=-1, keepdims=True))
    A = np.einsum("lnk,bok->lnbo", np.abs(w), np.abs(a) + np.abs(a).mean(axis=-1, keepdims=True))
    return G, A


def truth_and_bound(post, W_out, answers, scale):
    """float64 [B, T, L * M, O] each, from float32 inputs of a case's layout"""
    L, B, T, M = post.shape
    d = W_out.shape[-1]
    G, A = folded(W_out, answers, B)
    sc = scale.astype(np.float64)[None, :, :, None, None]
    p = post.astype(np.float64)[..., None]                                          # [L, B, T, M, 1]
    fin = np.isfinite(p)
    with np.errstate(invalid="ignore", over="ignore"):
        truth = np.where(fin, np.where(fin, p, 0.0) * G.transpose(0, 2, 1, 3)[:, :, None] / sc, np.nan)
        bound = (2 * d + 8) * U24 * np.where(fin, np.abs(p), 0.0) * A.transpose(0, 2, 1, 3)[:, :, None] / sc
    O = truth.shape[-1]
    # [L, B, T, M, O] -> [B, T, L * M, O]
    return (np.ascontiguousarray(truth.transpose(1, 2, 0, 3, 4)).reshape(B, T, L * M, O),
            np.ascontiguousarray(bound.transpose(1, 2, 0, 3, 4)).reshape(B, T, L * M, O))


@functools.lru_cache(maxsize=None)
def make_case(shape: tuple, per_image: bool, seed: int = 0) -> Case:
    B, T, L, M, d, O = shape
    assert T > TOK_SPARSE + 1 and B >= 2 and M >= 40
    rng = np.random.default_rng(1000 * seed + 7 * B + 11 * T + 13 * L + 17 * M + 23 * d + 29 * O + int(per_image))
    scale = (0.5 + 1.5 * rng.random((B, T))).astype(np.float32)
    answers = (0.05 * rng.standard_normal((B, O, d)) + 0.02).astype(np.float32)
    if per_image:
        answers[1] = -answers[0]
    else:
        answers = np.ascontiguousarray(answers[0])
    W_out = rng.standard_normal((L, M, d)) * 0.5 * M ** -0.5
    a0 = (answers[0] if per_image else answers).astype(np.float64)
    tie_row = (a0 - a0.mean(axis=-1, keepdims=True)).sum(axis=0)
    for l, n in tie_neurons(L, M):
        W_out[l, n] = tie_row
    W_out = bf16(W_out)
    post = rng.standard_normal((L, B, T, M)) * (1.0 + 0.25 * np.arange(L))[:, None, None, None]
    post[:, :, TOK_OUTLIER, [1, M // 2, M - 3]] = 30.0 * np.array([1.0, -1.0, 1.0])
    for l, n in tie_neurons(L, M):
        post[l, :, TOK_TIE, n] = TIE_POST
    post[:, :, TOK_SPARSE] = 0.0
    G0 = np.einsum("lnk,k->ln", W_out.astype(np.float64), a0[0] - a0[0].mean())                    # column 0 of image 0
    for l, n, sign, mag in sparse_neurons(L, M):
        post[l, :, TOK_SPARSE, n] = sign * mag * (1.0 if G0[l, n] >= 0 else -1.0)
    post = bf16(post)
    (ln, nn), (li, ni) = nonfinite_neurons(L, M)
    post[ln, :, TOK_NONFINITE, nn] = np.nan
    post[li, :, TOK_NONFINITE, ni] = np.inf
    if per_image:
        post[:, 1] = post[:, 0]
        scale[1] = scale[0]
    truth, bound = truth_and_bound(post, W_out, answers, scale)
    nan = np.zeros((B, T, L, M), bool)
    nan[:, TOK_NONFINITE, ln, nn] = True
    nan[:, TOK_NONFINITE, li, ni] = True
    zero = np.ascontiguousarray((post == 0).transpose(1, 2, 0, 3))
    return Case(shape, per_image, post, W_out, answers, scale, truth, bound, nan.reshape(B, T, L * M), zero.reshape(B, T, L * M))


def select_pos(a: np.ndarray, pos: int) -> np.ndarray:
    """[B, T, ...] -> what a call with `pos` returns: every token (pos = -1) or token `pos` alone, [B, 1, ...]"""
    return a if pos < 0 else a[:, pos:pos + 1]


def uncentred(case: Case) -> np.ndarray:
    """The form that forgets the centring, post (W_out[n] . a) / scale in float64: a kernel must NOT compute this."""
    L, B, T, M = case.post.shape
    a = case.answers.astype(np.float64)
    a = a if a.ndim == 3 else np.broadcast_to(a, (B, *a.shape))
    G = np.einsum("lnk,bok->lbno", case.W_out.astype(np.float64), a)                                # [L, B, M, O]
    with np.errstate(invalid="ignore", over="ignore"):
        out = case.post.astype(np.float64)[..., None] * G[:, :, None] / case.scale.astype(np.float64)[None, :, :, None, None]
    return np.ascontiguousarray(out.transpose(1, 2, 0, 3, 4)).reshape(B, T, L * M, -1)


def reference_composition(case: Case) -> np.ndarray:
    """The reference's composition, literally, in float64: the neuron results post[..., n, None] * W_out[n], centred over d_model,
    divided by the scale, times the answers -- [B, T, L * M, O].  For small cases only: it holds [B, T, M, d] per layer."""
    L, B, T, M = case.post.shape
    a = case.answers.astype(np.float64)
    a = a if a.ndim == 3 else np.broadcast_to(a, (B, *a.shape))
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(L):
            r = case.post[l].astype(np.float64)[..., None] * case.W_out[l].astype(np.float64)       # [B, T, M, d]
            r = (r - r.mean(axis=-1, keepdims=True)) / case.scale.astype(np.float64)[:, :, None, None]
            out.append(np.einsum("btnk,bok->btno", r, a))
    return np.concatenate(out, axis=2)


def topk_order(values: np.ndarray, k: int, by: int) -> np.ndarray:
    """values float32 [..., C, O] -> int64 [..., O, k]: the oracle's flat indices, largest key first"""
    v = np.moveaxis(np.asarray(values, dtype=np.float32), -1, -2)                                    # [..., O, C]
    isnan = np.isnan(v)
    key = np.where(isnan, np.float32(0), np.abs(v) if by else v) + np.float32(0)                      # (-0 + 0 = +0)
    index = np.broadcast_to(np.arange(v.shape[-1]), v.shape)
    order = np.lexsort((index, -key, ~isnan), axis=-1)                                               # the LAST key is the primary one
    return order[..., :k]
