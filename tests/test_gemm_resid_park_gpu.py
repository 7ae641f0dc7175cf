"""The residual park of the full-line GEMM (csrc/gemm_tiled.hpp, ResidParkSrc): gemm_kernel_v7<bf16, MB, RESID, 0, 2> fetches the residual
rows of its blocks 1 .. MB-1 with the DMA pieces that run off the end of its K loop, into LDS, and its store epilogue reads each
16-byte chunk back from where the same lane's DMA put it.

All through pv_gemm_epilogue with the kernel forced by the tuning overrides (gemm_tile 5 / 4, gemm_persist 0; gemm_loop stays
automatic: every K here is whole 128-byte slabs, so the full-line form runs).  Each launch is compared

    bit for bit   with the same launch on gemm_kernel_v4 (gemm_tile 0, residual rows in registers from before its K loop):
                  the tap (out0) and the residual sum (out1);
    in value      with the fp32 product: one bf16 rounding, 2^-8 of the row's largest entry, for out0 against A B^T + bias and for
                  out1 against out0 + residual (the bound of test_gemm_mfma_shape_gpu.py).

Shapes, each for what can break:

    M   320, 321, 351, 353, 639, 673 (MB = 5: 320-row tiles, a wave owns 160 rows in five blocks of 32) and 256, 257, 511 (MB = 4):
        a ragged last tile; a last tile whose second row half, or whose blocks 1 .., lie wholly past M (321, 351: block 0 of wave
        row 0 is partly real, block 1 is not; 353: block 1 has one real row); 639, 511: one row short of full.
    N   256, 264, 768: one tile column; a second one with a single live 8-column chunk (every other chunk of the tile dead);
        three full ones.
    K   64, 128, 192, 256, 384, 768: one, two, three, four, six and twelve 128-byte slabs -- with one or two the dead pieces are the
        prologue's and the tail step's, an odd count swaps the two ring slots' roles.
    ldr = N + 24: the residual's rows are longer than the output's.

The residual is PLANTED: the 8 values of the chunk at (row r, chunk c) are the hex digits of r and c (integers 0 .. 15, exact in
bf16), so no two chunks of the matrix are alike and a chunk read from another lane's or another wave's slot changes at least one sum
by >= 1 where out0 is kept below 4 (bf16 steps of at most 1/8 there).  The residual's padding columns and the rows behind row M are
NaN; the outputs carry guard rows up to the next tile boundary that must stay as they were.

(The ViT plan never hands the kernel a residual that aliases out1 -- vit_plan.hip: resid_pre -> resid_mid -> resid_post are three
buffers -- so that case is not among these.)
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from vit_prisma_amd import _native

pytestmark = pytest.mark.gpu

NS = (256, 264, 768)
KS = (64, 128, 192, 256, 384, 768)
M_MAX = 673
GUARD = 7.0
_cache: dict = {}


def _operands(N, K):
    """A (M_MAX x K), B (N x K), bias and the fp32 product of the whole problem: made once per (N, K), never written again."""
    if (N, K) not in _cache:
        g = torch.Generator(device="cuda").manual_seed(7000 + N + K)
        A = torch.randn(M_MAX, K, device="cuda", generator=g).bfloat16()
        B = (torch.randn(N, K, device="cuda", generator=g) * (0.4 / K ** 0.5)).bfloat16()      # |A B^T| ~ 0.4
        bias = (torch.randn(N, device="cuda", generator=g) * 0.2).bfloat16()
        pre = (A.double() @ B.double().T + bias.double()).float()
        _cache[(N, K)] = (A, B, bias, pre)
    return _cache[(N, K)]


def _planted_residual(M, N, ldr, rows_alloc):
    """[rows_alloc][ldr] bf16: chunk (r, c) = hex digits of r (3) and of c (2), then r + c, r ^ c, 1; NaN in the padding and behind M."""
    r = torch.arange(M, device="cuda").view(M, 1, 1)
    c = torch.arange(N // 8, device="cuda").view(1, N // 8, 1)
    digits = torch.cat([(r >> s & 15).expand(M, N // 8, 1) for s in (0, 4, 8)] + [(c >> s & 15).expand(M, N // 8, 1) for s in (0, 4)] +
                       [((r + c) & 15), ((r ^ c) & 15), torch.ones_like(r + c)], dim=2)
    res = torch.full((rows_alloc, ldr), float("nan"), device="cuda", dtype=torch.bfloat16)
    res[:M, :N] = digits.reshape(M, N).to(torch.bfloat16)
    return res


def _launch(A, B, bias, res, ldr, M, N, K, rows_alloc):
    L = _native.lib()
    st = torch.cuda.current_stream().cuda_stream
    o0 = torch.full((rows_alloc, N), GUARD, device="cuda", dtype=torch.bfloat16)
    o1 = torch.full((rows_alloc, N), GUARD, device="cuda", dtype=torch.bfloat16)
    _native.check(L.pv_gemm_epilogue(1, 2, 0, A.data_ptr(), K, B.data_ptr(), K, bias.data_ptr(), res.data_ptr(), ldr,
                                     o0.data_ptr(), o1.data_ptr(), N, M, N, K, st), "pv_gemm_epilogue")
    torch.cuda.synchronize()
    return o0, o1


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("tile,M", [(5, 320), (5, 321), (5, 351), (5, 353), (5, 639), (5, 673), (4, 256), (4, 257), (4, 511)])
def test_parked_residual_same_bits_as_v4_and_within_bf16_rounding(tile, M, tuning):
    tm = 64 * tile
    rows_alloc = (M + tm - 1) // tm * tm + 8
    for N in NS:
        ldr = N + 24
        res = _planted_residual(M, N, ldr, rows_alloc)
        chunks = res[:M, :N].reshape(M * (N // 8), 8).float()
        assert torch.unique(chunks, dim=0).shape[0] == M * (N // 8)                 # no two chunks alike
        for K in KS:
            A, B, bias, pre = _operands(N, K)
            A = A[:M].contiguous()
            tuning("reset")
            tuning("gemm_tile", tile)
            tuning("gemm_persist", 0)
            p0, p1 = _launch(A, B, bias, res, ldr, M, N, K, rows_alloc)
            tuning("reset")
            tuning("gemm_tile", 0)
            v0, v1 = _launch(A, B, bias, res, ldr, M, N, K, rows_alloc)
            tuning("reset")
            where = (tile, M, N, K)
            for got, ref, name in ((p0, v0, "out0"), (p1, v1, "out1")):
                assert bool((got[M:].float() == GUARD).all()) and bool((ref[M:].float() == GUARD).all()), (where, name, "guard rows")
                bad = (_bits(got[:M]) != _bits(ref[:M])).nonzero()
                assert bad.numel() == 0, (where, name, bad[:4].tolist(), len(bad))
            assert not bool(torch.isnan(p1[:M].float()).any()), where
            want0 = pre[:M]
            want1 = p0[:M].float() + res[:M, :N].float()
            for got, want, name in ((p0[:M], want0, "out0"), (p1[:M], want1, "out1")):
                worst = float(((got.float() - want).abs().amax(dim=1) / want.abs().amax(dim=1)).max())
                assert worst < 2.0 ** -8, (where, name, worst)
            assert float(p0[:M].float().abs().max()) < 4.0, where                    # (what makes a foreign chunk visible)


def test_the_forced_launch_is_the_full_line_v7_kernel(tuning):
    """The tuning keys above really select gemm_kernel_v7 (the trace records which kernel a launch went to) and the launch's
    workgroups all ran to their end."""
    L = _native.lib()
    L.pv_debug_gemm_trace_arm.argtypes = [ctypes.c_int32]
    L.pv_debug_gemm_trace_read.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
    M, N, K = 353, 264, 192
    A, B, bias, _ = _operands(N, K)
    res = _planted_residual(M, N, N + 24, 648)
    for tile, tiles in ((5, 4), (4, 4)):
        tuning("reset")
        tuning("gemm_tile", tile)
        tuning("gemm_persist", 0)
        assert L.pv_debug_gemm_trace_arm(0) == 0
        _launch(A[:M].contiguous(), B, bias, res, N + 24, M, N, K, 648)
        buf = np.zeros((64, 4), np.uint64)
        info = np.zeros(6, np.int32)
        assert L.pv_debug_gemm_trace_read(buf.ctypes.data, 64, info.ctypes.data) == 0
        tuning("reset")
        assert info.tolist() == [M, N, K, 2, tiles, 70 + tile]
        assert (buf[:tiles, 2] > buf[:tiles, 1]).all() and (buf[:tiles, 1] > buf[:tiles, 0]).all()


# ---- the trace describes the launch that happened: its info comes from the choice that launched (csrc/gemm.hip, choose()), also
# ---- where the forced tile is not what the launch can take

def _traced(tuning, keys, A, B, bias, res, lda, ldr, M, N, K, rows_alloc=648):
    """One armed launch under the tuning keys: (out0, out1, the first 64 rows of the trace buffer, info)."""
    L = _native.lib()
    L.pv_debug_gemm_trace_arm.argtypes = [ctypes.c_int32]
    L.pv_debug_gemm_trace_read.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
    st = torch.cuda.current_stream().cuda_stream
    o0 = torch.full((rows_alloc, N), GUARD, device="cuda", dtype=torch.bfloat16)
    o1 = torch.full((rows_alloc, N), GUARD, device="cuda", dtype=torch.bfloat16)
    tuning("reset")
    for key, value in keys.items():
        tuning(key, value)
    assert L.pv_debug_gemm_trace_arm(0) == 0
    rc = L.pv_gemm_epilogue(1, 2, 0, A.data_ptr(), lda, B.data_ptr(), lda, bias.data_ptr(), res.data_ptr(), ldr,
                            o0.data_ptr(), o1.data_ptr(), N, M, N, K, st)
    buf = np.zeros((64, 4), np.uint64)
    info = np.zeros(6, np.int32)
    rc_read = L.pv_debug_gemm_trace_read(buf.ctypes.data, 64, info.ctypes.data)
    tuning("reset")
    _native.check(rc, "pv_gemm_epilogue")
    assert rc_read == 0
    return o0, o1, buf, info.tolist()


def _stamped_in_order(rows):
    return bool(((rows[:, 2] > rows[:, 1]) & (rows[:, 1] > rows[:, 0]) & (rows[:, 0] > 0)).all())


def test_trace_of_a_forced_tile_that_falls_back_to_v4(tuning):
    """ldr = N + 4: the residual's rows are no 16-byte multiples, the vector epilogue is not legal and the launch is gemm_kernel_v4's
    on 3 x 3 tiles of 128 x 128, whatever gemm_tile says -- and that is what the trace must say (it used to say kernel 75 on 4
    workgroups, and the 8192-row guard was applied to that count)."""
    M, N, K = 353, 264, 192
    A, B, bias, _ = _operands(N, K)
    A = A[:M].contiguous()
    res = _planted_residual(M, N, N + 4, 648)
    o0, o1, buf, info = _traced(tuning, {"gemm_tile": 5, "gemm_persist": 0}, A, B, bias, res, K, N + 4, M, N, K)
    print("info", info, "rows stamped", int((buf[:, 0] > 0).sum()))
    assert info == [M, N, K, 2, 3 * 3, 4]
    assert _stamped_in_order(buf[:9]), buf[:9]
    assert not buf[9].any(), buf[9]
    tuning("gemm_tile", 0)
    v0, v1 = _launch(A, B, bias, res, N + 4, M, N, K, 648)
    tuning("reset")
    for got, ref, name in ((o0, v0, "out0"), (o1, v1, "out1")):
        assert bool((_bits(got) == _bits(ref)).all()), name


def test_trace_of_a_launch_that_falls_back_to_gemm_kernel(tuning):
    """K = 100, lda = ldb = 100: 200-byte operand rows are not 16-byte legal, the launch is gemm_kernel's, which writes no stamps:
    kernel 1, no workgroups, nothing in the buffer (the info used to describe a v7 launch, and the zeros read as its trace)."""
    M, N, K = 353, 264, 100
    g = torch.Generator(device="cuda").manual_seed(7100)
    A = torch.randn(M, K, device="cuda", generator=g).bfloat16()
    B = (torch.randn(N, K, device="cuda", generator=g) * (0.4 / K ** 0.5)).bfloat16()
    bias = (torch.randn(N, device="cuda", generator=g) * 0.2).bfloat16()
    pre = (A.double() @ B.double().T + bias.double()).float()
    res = _planted_residual(M, N, N + 4, 648)
    o0, o1, buf, info = _traced(tuning, {"gemm_tile": 5, "gemm_persist": 0}, A, B, bias, res, K, N + 4, M, N, K)
    print("info", info)
    assert info[:4] == [M, N, K, 2] and info[4] == 0 and info[5] == 1, info
    assert not buf.any()
    assert bool((o0[M:].float() == GUARD).all()) and bool((o1[M:].float() == GUARD).all())
    for got, want, name in ((o0[:M], pre, "out0"), (o1[:M], o0[:M].float() + res[:M, :N].float(), "out1")):
        worst = float(((got.float() - want).abs().amax(dim=1) / want.abs().amax(dim=1)).max())
        print(name, "worst", worst)
        assert worst < 2.0 ** -8, (name, worst)


def test_trace_of_the_persistent_kernel(tuning):
    """gemm_persist 1, four 128-byte slabs: gemm_kernel_v8, whose stamps are indexed by virtual block id -- one row per tile."""
    M, N, K = 353, 264, 256
    A, B, bias, _ = _operands(N, K)
    res = _planted_residual(M, N, N + 24, 648)
    _, _, buf, info = _traced(tuning, {"gemm_tile": 5, "gemm_persist": 1}, A[:M].contiguous(), B, bias, res, K, N + 24, M, N, K)
    print("info", info)
    assert info == [M, N, K, 2, 4, 75]
    assert _stamped_in_order(buf[:4]), buf[:4]
