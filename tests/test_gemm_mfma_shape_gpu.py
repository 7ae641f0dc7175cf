"""The bf16 GEMM kernels on v_mfma_f32_16x16x32_bf16 (csrc/kloop.hpp, csrc/gemm_tiled.hpp, csrc/gemm_v4.hpp): fragment and accumulator lane maps, and that
every kernel / K-loop form accumulates alike.

All through pv_gemm_epilogue with the kernel forced by the tuning overrides, on the smallest shapes that cross every boundary:

    M = 333, N = 264   one full 320 x 256 (256 x 256) tile, ragged rows, one extra 8-column chunk      gemm_tile 4, 5
    M = 130, N = 136   the same for the 128 x 128 kernel (the top-left block of the same problem)       gemm_tile 0
    M = 1300, N = 264  more tiles than gemm_cus = 8: the persistent kernel walks                        gemm_persist 1, K = 128
    K = 40             ends inside a 64-byte slab: the barrier-then-fetch loop
    K = 96             three 64-byte slabs: the pipelined loop
    K = 128            two whole cache lines: the full-line loop; the persistent kernel
    K = 192            an odd number of them: the full-line loop, never persistent
    gemm_loop 0, 1, 2  a form that is not legal for a K falls back to the next simpler one

EXACT: operands, bias and residual are integers in -3 .. 3, so every product and every partial sum is exact in fp32 whatever the
order (|sum| <= 9 * 192 + 3) and the outputs must EQUAL the fp64 product rounded where the epilogue rounds: bias -> round; residual:
round, + residual, round; activation (ReLU, exact): round, max(., 0).  A lane map that is off by one register shows here.

RANDOM: the same settings on randn operands must give the same bits as each other (one k order for every output, whatever the
kernel), and stay within one bf16 rounding -- 2^-8 of the row's largest entry -- of the fp32 product + bias (out0) and of the
epilogue's own function of the stored out0 (out1: + residual / GELU).
"""
from __future__ import annotations

import pytest
import torch

from vit_prisma_amd import _native

pytestmark = pytest.mark.gpu

M_BIG, N_BIG = 333, 264
M_V4, N_V4 = 130, 136
M_PERSIST = 1300
EPI = {"bias": 0, "resid": 2, "act": 3}


def _run(epi, act, A, B, bias, res):
    M, K = A.shape
    N = B.shape[0]
    L = _native.lib()
    st = torch.cuda.current_stream().cuda_stream
    o0 = torch.full((M + 1, N), 7.0, device="cuda", dtype=torch.bfloat16)             # the extra row must stay untouched
    o1 = torch.full((M + 1, N), 7.0, device="cuda", dtype=torch.bfloat16) if epi != "bias" else None
    _native.check(L.pv_gemm_epilogue(1, EPI[epi], act, A.data_ptr(), K, B.data_ptr(), K, bias.data_ptr(),
                                     res.data_ptr() if epi == "resid" else None, N, o0.data_ptr(),
                                     o1.data_ptr() if o1 is not None else None, N, M, N, K, st), "pv_gemm_epilogue")
    torch.cuda.synchronize()
    for o in (o0, o1):
        if o is not None:
            assert float(o[M].float().min()) == 7.0 and float(o[M].float().max()) == 7.0
    return o0[:M], (o1[:M] if o1 is not None else None)


def _all_settings(tuning, epi, act, K, A, B, bias, res):
    """{setting: (out0, out1)} of the (M_BIG, N_BIG) problem; the gemm_tile = 0 and the persistent entries cover other row ranges."""
    outs = {}
    for tile in (4, 5):
        for loop in (0, 1, 2):
            tuning("reset")
            tuning("gemm_tile", tile)
            tuning("gemm_loop", loop)
            tuning("gemm_persist", 0)
            outs[(tile, loop)] = _run(epi, act, A[:M_BIG], B, bias, res[:M_BIG])
    tuning("reset")
    tuning("gemm_tile", 0)
    outs["v4"] = _run(epi, act, A[:M_V4].contiguous(), B[:N_V4].contiguous(), bias[:N_V4].contiguous(),
                      res[:M_V4, :N_V4].contiguous())
    if K == 128:
        for tile in (4, 5):
            tuning("reset")
            tuning("gemm_tile", tile)
            tuning("gemm_persist", 1)
            tuning("gemm_cus", 8)
            outs[("persist", tile)] = _run(epi, act, A, B, bias, res)
    tuning("reset")
    return outs


def _block(key, t):
    """The part of the reference / of another setting's result that setting `key` computed."""
    if key == "v4":
        return t[:M_V4, :N_V4]
    return t if isinstance(key[0], str) else t[:M_BIG]


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("K", [40, 96, 128, 192])
@pytest.mark.parametrize("epi", ["bias", "resid", "act"])
def test_small_integer_operands_give_the_exact_product_in_every_kernel(epi, K, tuning):
    g = torch.Generator(device="cuda").manual_seed(1000 + K)

    def ints(*shape):
        return torch.randint(-3, 4, shape, device="cuda", generator=g).to(torch.bfloat16)

    A, B, bias, res = ints(M_PERSIST, K), ints(N_BIG, K), ints(N_BIG), ints(M_PERSIST, N_BIG)
    pre = (A.double() @ B.double().T + bias.double()).to(torch.bfloat16)              # exact, then the epilogue's first rounding
    want0 = pre
    if epi == "resid":
        want1 = (pre.double() + res.double()).to(torch.bfloat16)
    elif epi == "act":
        want1 = torch.clamp_min(pre.float(), 0.0).to(torch.bfloat16)
    else:
        want1 = None
    outs = _all_settings(tuning, epi, 2, K, A, B, bias, res)                          # 2 = PV_ACT_RELU
    assert len(outs) == (9 if K == 128 else 7)
    for key, (o0, o1) in outs.items():
        bad = (o0.float() != _block(key, want0).float()).nonzero()
        assert bad.numel() == 0, (key, "out0", bad[:4].tolist(), len(bad))
        if want1 is not None:
            bad = (o1.float() != _block(key, want1).float()).nonzero()
            assert bad.numel() == 0, (key, "out1", bad[:4].tolist(), len(bad))


@pytest.mark.parametrize("K", [40, 96, 128, 192])
@pytest.mark.parametrize("epi", ["bias", "resid", "act"])
def test_random_operands_same_bits_in_every_kernel_and_within_bf16_rounding(epi, K, tuning):
    g = torch.Generator(device="cuda").manual_seed(2000 + K)
    A = torch.randn(M_PERSIST, K, device="cuda", generator=g).bfloat16()
    B = (torch.randn(N_BIG, K, device="cuda", generator=g) * 0.05).bfloat16()
    bias = torch.randn(N_BIG, device="cuda", generator=g).bfloat16()
    res = torch.randn(M_PERSIST, N_BIG, device="cuda", generator=g).bfloat16()
    outs = _all_settings(tuning, epi, 0, K, A, B, bias, res)                          # 0 = PV_ACT_GELU
    ref_key = ("persist", 5) if K == 128 else (5, 2)                                  # (the persistent run covers every row range)
    r0, r1 = outs[ref_key]
    for key, (o0, o1) in outs.items():
        assert torch.equal(_bits(o0), _bits(_block(key, r0))), (key, "out0")
        if o1 is not None:
            assert torch.equal(_bits(o1), _bits(_block(key, r1))), (key, "out1")

    def close(got, want):
        worst = float(((got.float() - want).abs().amax(dim=1) / want.abs().amax(dim=1)).max())
        print(f"{epi} K={K}: {worst:.3e} of the row's largest entry (bound {2.0 ** -8:.3e})")
        return worst < 2.0 ** -8

    rows = r0.shape[0]
    pre = (A[:rows].double() @ B.double().T + bias.double()).float()
    assert close(r0, pre)
    if epi == "resid":
        assert close(r1, r0.float() + res[:rows].float())
    if epi == "act":
        assert close(r1, torch.nn.functional.gelu(r0.float()))
