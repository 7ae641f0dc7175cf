"""Planted inputs for pv_head_attribution (csrc/attribution.hip), their float64 truth and the per-element bound.  No GPU needed here.

A case is L taps z [B, T, H, d_head] and L matrices W_O [H, d_head, d] (both bf16-representable, distinct per layer), fp32 answers
(NOT bf16-representable: 0.05 x Gaussian + 0.02, the offset so that centring matters) and a positive fp32 scale [B, T].  Shared
answers are [O, d]; per-image answers are [B, O, d] with image 1's the exact negation of image 0's, and then image 1 also holds
image 0's z and scale, so that its outputs must be the exact negatives of image 0's -- which they are only if the kernel picks
the answers by the row's image.

Tokens (in every image and layer):  0 plain Gaussian | 1 head 0 has three outlier channels at 30 x | 2 head 1 is zero: exactly 0
in every column | 3 head 0 holds one NaN | 4 head 1 holds one +inf -- both NaN in all their columns, the other heads of those rows
finite and within the bound | from 5 on plain.

Truth, float64:  out[b, t, l H + h, o] = ((r - mean(r)) . a_o) / scale[b, t],  r = z[l, b, t, h, :] @ W_O[l, h].

Bound for ANY fp32 summation order of the folded form  (sum_e z_e G_e) / scale,  G_e = sum_k W_ek ac_k,  ac = a - mean(a)
(u = 2^-24; bf16 x fp32 products are not exact in fp32, so every product rounds once as well):
  * mean(a): a sum of d terms and one division: |m^ - m| <= (d + 1) u mean|a| to first order; ac^_k = fl(a_k - m^) adds one
    rounding: |ac^_k - ac_k| <= u |ac_k| + (d + 1) u mean|a| <= (d + 2) u (|a_k| + mean|a|), and |ac_k| <= |a_k| + mean|a|
  * G_e: d products and a sum of d terms in some order: relative (d + 1) u on sum_k |W_ek| |ac^_k|
  * the dot product: d_head products and a sum of d_head terms: relative (d_head + 1) u on sum_e |z_e| |G^_e|; the division: u
  together, to first order, with A_e = sum_k |W_ek| (|a_k| + mean_k |a_k|):
    |got - truth| <= ((d + 2) + (d + 1) + (d_head + 1) + 1) u sum_e |z_e| A_e / scale <= (2 d + d_head + 8) u sum_e |z_e| A_e / scale
  The constant 2 d + d_head + 8 leaves 3 u for the second-order terms.  The kernels add every product with one fused
  multiply-add (one rounding per term, not two), which is inside this count.  Derived, not measured.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np
import torch

U24 = 2.0 ** -24
# (B, T, L, H, d_head, d, O)
SHAPES = [
    (3, 5, 2, 3, 32, 96, 1),          # images shorter than any row tile
    (2, 50, 3, 12, 64, 768, 4),       # the bench geometry
    (2, 197, 2, 12, 64, 768, 16),     # several row tiles per image; the answer cap
    (2, 7, 2, 4, 80, 320, 3),         # a wide head
    (2, 7, 1, 2, 104, 208, 16),       # a wide head at the answer cap
    (2, 7, 1, 2, 72, 144, 3),         # the narrowest wide head (the rule serves every multiple of 8 in (64, 128])
]
TOK_OUTLIER, TOK_ZERO, TOK_NAN, TOK_INF = 1, 2, 3, 4
HEAD_OUTLIER, HEAD_ZERO, HEAD_NAN, HEAD_INF = 0, 1, 0, 1


def shape_id(shape) -> str:
    return "B{}-T{}-L{}-H{}-dh{}-d{}-O{}".format(*shape)


def bf16(a: np.ndarray) -> np.ndarray:
    """round to bf16 (nearest even), back as float32"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy()


@dataclass
class Case:
    shape: tuple
    per_image: bool
    z: np.ndarray               # [L, B, T, H, d_head] float32, bf16-representable (NaN / inf planted)
    W_O: np.ndarray             # [L, H, d_head, d] float32, bf16-representable
    answers: np.ndarray         # [O, d] or [B, O, d] float32
    scale: np.ndarray           # [B, T] float32, positive
    truth: np.ndarray           # [B, T, L * H, O] float64 (NaN in the planted heads)
    bound: np.ndarray           # [B, T, L * H, O] float64
    nan: np.ndarray             # [B, T, L * H] bool: heads that must be NaN in every column
    zero: np.ndarray            # [B, T, L * H] bool: heads that must be exactly 0 in every column


def truth_and_bound(z, W_O, answers, scale):
    """float64 [B, T, L * H, O] each, from float32 inputs of a case's layout"""
    L, B, T, H, dh = z.shape
    d = W_O.shape[-1]
    a = answers.astype(np.float64)
    if a.ndim == 2:
        a = np.broadcast_to(a, (B, *a.shape))
    sc = scale.astype(np.float64)[:, :, None, None]
    amag = np.abs(a) + np.abs(a).mean(axis=-1, keepdims=True)                       # [B, O, d]
    truth, bound = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(L):
            z64, w64 = z[l].astype(np.float64), W_O[l].astype(np.float64)
            r = np.einsum("bthe,hek->bthk", z64, w64)
            rc = r - r.mean(axis=-1, keepdims=True)
            truth.append(np.einsum("bthk,bok->btho", rc, a) / sc)
            A = np.einsum("hek,bok->bheo", np.abs(w64), amag)                       # [B, H, d_head, O]
            zabs = np.where(np.isfinite(z64), np.abs(z64), 0.0)
            bound.append((2 * d + dh + 8) * U24 * np.einsum("bthe,bheo->btho", zabs, A) / sc)
    return np.concatenate(truth, axis=2), np.concatenate(bound, axis=2)


@functools.lru_cache(maxsize=None)
def make_case(shape: tuple, per_image: bool, seed: int = 0) -> Case:
    B, T, L, H, dh, d, O = shape
    assert T > TOK_INF and H >= 2 and B >= 2
    rng = np.random.default_rng(1000 * seed + 7 * B + 11 * T + 13 * L + 17 * H + 19 * dh + 23 * d + 29 * O + int(per_image))
    W_O = bf16(rng.standard_normal((L, H, dh, d)) * 0.5 * (H * dh) ** -0.5)
    z = rng.standard_normal((L, B, T, H, dh)) * (1.0 + 0.25 * np.arange(L))[:, None, None, None, None]
    z[:, :, TOK_OUTLIER, HEAD_OUTLIER, [1, dh // 2, dh - 3]] = 30.0 * np.array([1.0, -1.0, 1.0])
    z[:, :, TOK_ZERO, HEAD_ZERO] = 0.0
    z = bf16(z)
    z[:, :, TOK_NAN, HEAD_NAN, dh // 3] = np.nan
    z[:, :, TOK_INF, HEAD_INF, dh // 5] = np.inf
    scale = (0.5 + 1.5 * rng.random((B, T))).astype(np.float32)
    answers = (0.05 * rng.standard_normal((B, O, d)) + 0.02).astype(np.float32)
    if per_image:
        answers[1] = -answers[0]
        z[:, 1] = z[:, 0]
        scale[1] = scale[0]
    else:
        answers = np.ascontiguousarray(answers[0])
    truth, bound = truth_and_bound(z, W_O, answers, scale)
    nan = np.zeros((B, T, L, H), bool)
    nan[:, TOK_NAN, :, HEAD_NAN] = True
    nan[:, TOK_INF, :, HEAD_INF] = True
    zero = np.zeros((B, T, L, H), bool)
    zero[:, TOK_ZERO, :, HEAD_ZERO] = True
    return Case(shape, per_image, z, W_O, answers, scale, truth, bound, nan.reshape(B, T, L * H), zero.reshape(B, T, L * H))


def select_pos(a: np.ndarray, pos: int) -> np.ndarray:
    """[B, T, ...] -> what a call with `pos` returns: every token (pos = -1) or token `pos` alone, [B, 1, ...]"""
    return a if pos < 0 else a[:, pos:pos + 1]


def uncentred(case: Case) -> np.ndarray:
    """The form that forgets the centring, (r . a) / scale in float64: a kernel must NOT compute this."""
    L, B, T, H, dh = case.z.shape
    a = case.answers.astype(np.float64)
    a = a if a.ndim == 3 else np.broadcast_to(a, (B, *a.shape))
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(L):
            r = np.einsum("bthe,hek->bthk", case.z[l].astype(np.float64), case.W_O[l].astype(np.float64))
            out.append(np.einsum("bthk,bok->btho", r, a) / case.scale.astype(np.float64)[:, :, None, None])
    return np.concatenate(out, axis=2)
