"""The planted inputs of tests/_rowop_cases.py have the properties they claim, float32 CPU twins of the kernels (their order of
operations, exact exp2 / reciprocal) and torch fp32 of the reference's formulas pass the checkers, twins that are wrong on purpose fail
them, and the assertions the GPU suite had before accept those wrong twins.  No GPU."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import _rowop_cases as RC

ROWS = 15                                                # B = 3 images x T = 5 tokens: the last 4-row workgroup holds 3
WIDTHS = (8, 136, 520, 1032, 1544, 2048)                 # what tests/test_rowops_adversarial_gpu.py runs
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def _rows(name, d):
    return RC.ln_rows(name, ROWS, d)


@functools.lru_cache(maxsize=None)
def _twin(name, d, planted=True, fma=True, bug=None):
    w, b = RC.ln_weights(d, planted)
    return RC.ln_twin(_rows(name, d), w, b, fma=fma, bug=bug)


def _check_twin(name, d, planted=True, fma=True, bug=None):
    w, b = RC.ln_weights(d, planted)
    s, y, y16 = _twin(name, d, planted, fma, bug)
    return RC.check_ln(_rows(name, d), w, b, scale=s, y32=y, y16=y16)


# ------------------------------------------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("d", WIDTHS)
def test_ln_cases_have_the_properties_they_claim(d):
    w, b = RC.ln_weights(d)
    assert bool((w.bfloat16().float() == w).all() and (b.bfloat16().float() == b).all()) and float(w.std()) > 0.2
    for name in RC.LN_CASES:
        x = _rows(name, d)
        assert x.shape == (ROWS, d) and bool(((x.bfloat16().float() == x) | torch.isnan(x)).all()), name
        ref = RC.ln_reference(x, w, b)
        good = torch.isfinite(x).all(-1)
        assert bool(good.all()) == (name != "nonfinite")
        assert bool(torch.isfinite(ref["scale"][good]).all() and torch.isfinite(ref["y"][good]).all() and (ref["A"][good] > 0).all()), name
        ratio, scale = ref["ratio"], ref["scale"]
        if name == "offset":
            assert sorted(set(x.flatten().tolist())) == [996.0, 1000.0, 1004.0]
            assert float(ratio.min()) > 280 and float(ratio.max()) < 500, (float(ratio.min()), float(ratio.max()))
        if name == "const":
            assert bool((x == x[:, :1]).all()) and len(set(x[:, 0].tolist())) > ROWS // 2 and float(x[:, 0].abs().max()) == 1000.0
            assert float((scale - math.sqrt(RC.LN_EPS)).abs().max()) < 1e-15 and bool((ref["y"] == b.double()).all())
            v = x[:, 0]
            assert bool(((8 * v) == (8 * v).round()).all()) and bool(((v.abs() < 8) | (v == 1000)).all())
            two = (v[:, None] + v[None, :]).flatten()                                    # an fp32 EMBED row: cls / bias + pos
            assert bool((two[:, None].expand(-1, 2048).contiguous().cumsum(-1) == two[:, None] * torch.arange(1, 2049)).all())     # exact in fp32
        if name == "massive":
            assert bool((x[:, 0] == 180).all() and (x[:, d - 1] == -300).all())
        if name == "outlier":
            hit = (x == 2.0 ** 14).nonzero()
            assert hit[:, 0].tolist() == list(range(ROWS)) and hit[:, 1].tolist() == [RC.outlier_channel(r, d) for r in range(ROWS)]
            if d >= 1032:
                assert len({c // 512 for c in hit[:, 1].tolist()}) > 1                    # more than one register chunk
        if name == "onehot_last":
            assert float(x.abs().sum()) == ROWS and bool((x[:, d - 1] == 1).all())
        if name == "tiny":
            assert float(x.abs().max()) < 2.0 ** -37 and float((scale / math.sqrt(RC.LN_EPS) - 1).abs().max()) < 1e-15
        if name == "huge":
            assert 2.0 ** 50 < float(x.abs().max()) < 2.0 ** 56 and math.isfinite(float(x.float().pow(2).sum(-1).max()))
        if name == "nonfinite":
            bad = RC.bad_ln_rows(ROWS)
            assert bad == [1, 6, 9, 14] and (~good).nonzero().flatten().tolist() == bad
            for g0 in range(0, ROWS, 4):                                                 # every workgroup: good rows beside a bad one
                assert 0 < int((~good[g0:g0 + 4]).sum()) < len(good[g0:g0 + 4])
            kinds = [(bool(torch.isnan(x[r]).any()), bool((x[r] == float("inf")).any()), bool((x[r] == float("-inf")).any())) for r in bad]
            assert kinds == [(True, False, False), (False, True, False), (False, False, True), (True, True, True)]
            t_scale, t_y = RC.ln_torch(x, w, b)                                          # the expectation: NaN throughout
            assert bool(torch.isnan(t_scale[~good]).all() and torch.isnan(t_y[~good]).all())
            assert bool(torch.equal(x[good], _rows("normal", d)[good]))


@pytest.mark.parametrize("d", WIDTHS)
def test_ln_twin_with_the_kernels_summation_order_passes_every_case_in_both_dtypes(d):
    """... and stays below HALF the bound on the fp32 quantities (4 u): the 8 of the bound was not chosen to fit it"""
    worst = {}
    for planted in (True, False):
        for name in RC.LN_CASES:
            for fma in (True, False):
                r = _check_twin(name, d, planted, fma)
                assert RC.passes(r) and r["scale"] < 0.5 and r["y32"] < 0.5, (name, planted, fma, r)
                s, y, y16 = _twin(name, d, planted, fma)
                assert torch.equal(y16.view(torch.int16), y.to(torch.bfloat16).view(torch.int16))
                for k, v in r.items():
                    worst[k] = max(worst.get(k, 0.0), v)
    print(RC.report(f"ln_twin d={d}", worst))


@pytest.mark.parametrize("d", WIDTHS)
def test_torch_fp32_of_the_reference_layer_norm_passes_every_case(d):
    worst = {}
    for planted in (True, False):
        w, b = RC.ln_weights(d, planted)
        for name in RC.LN_CASES:
            r = RC.ln_torch_ratios(_rows(name, d), w, b, bf16=True)
            assert RC.passes(r) and r["scale"] < 0.5 and r["y32"] < 0.5, (name, planted, r)
            for k, v in r.items():
                worst[k] = max(worst.get(k, 0.0), v)
    print(RC.report(f"torch fp32 d={d}", worst))


@pytest.mark.parametrize("d", [520, 2048])
@pytest.mark.parametrize("bug", RC.LN_BUGS)
def test_wrong_ln_twins_fail(bug, d):
    if bug == "divisor_512" and d == 2048:
        # 512 ceil(d / 512) IS d at 2048: this twin is the kernel there and can only be told apart at a ragged width
        for name in ("normal", "massive"):
            for a, c in zip(_twin(name, d, bug=bug), _twin(name, d)):
                assert torch.equal(a, c)
        return
    failed = {name: r for name in RC.LN_CASES for r in [_check_twin(name, d, bug=bug)] if not RC.passes(r)}
    print(f"{bug} d={d}: fails " + ", ".join(f"{n} ({max(r.values()):.3g})" for n, r in failed.items()))
    assert failed, bug
    must = {"one_pass": "offset", "no_eps": "const", "eps_after_sqrt": "const", "divisor_512": "normal", "skip_chunks_sum": "onehot_last",
            "skip_chunks_write": "normal", "wb_chunk0": "normal", "last_row_unwritten": "normal", "nan_neighbours": "nonfinite",
            "centred_in_bf16": "normal", "tap_from_bf16": "normal"}[bug]
    assert must in failed, (bug, must, sorted(failed))
    if bug == "nan_neighbours":
        assert sorted(failed) == ["nonfinite"]
    if bug == "tap_from_bf16":                            # only the fp32 tap is wrong: the bf16 output is the kernel's
        assert failed[must]["y32"] > 1 and failed[must]["y16"] <= 1 and failed[must]["scale"] <= 1


def test_a_tensor_wide_frobenius_norm_at_the_budgets_size_accepts_one_wrong_row():
    """What test_native_vit_gpu holds the LayerNorm taps to: a relative Frobenius norm per hook key, the reference's own bf16 error.
    One row of 15 whose sums skip every chunk but the first (d = 520: 8 of 520 elements missing from mean and variance) stays inside
    blocks.0.ln1.hook_normalized's budget, and one row whose eps is added behind the square root stays inside hook_scale's; the
    per-row, per-element bounds reject both."""
    with open(os.path.join(GOLDEN, "vit_b32_bf16_budget.json")) as f:
        budget = json.load(f)["budget"]
    d, row = 520, 7
    x = _rows("normal", d)
    w, b = RC.ln_weights(d)
    ref = RC.ln_reference(x, w, b)

    def fro(got, want):
        return float((got.double() - want).norm() / want.norm())

    s, y, _ = (t.clone() for t in _twin("normal", d))
    assert fro(y, ref["y"]) < 1e-6 and fro(s, ref["scale"]) < 1e-6
    y[row] = _twin("normal", d, bug="skip_chunks_sum")[1][row]
    s[row] = _twin("normal", d, bug="eps_after_sqrt")[0][row]
    e_y, e_s = fro(y, ref["y"]), fro(s, ref["scale"])
    print(f"one wrong row of {ROWS}: rel_fro hook_normalized {e_y:.3e} (budget {budget['blocks.0.ln1.hook_normalized']['rel_fro']:.3e}), "
          f"hook_scale {e_s:.3e} (budget {budget['blocks.0.ln1.hook_scale']['rel_fro']:.3e})")
    assert 1e-4 < e_y <= budget["blocks.0.ln1.hook_normalized"]["rel_fro"]
    assert 1e-7 < e_s <= budget["blocks.0.ln1.hook_scale"]["rel_fro"]
    r = RC.check_ln(x, w, b, scale=s, y32=y)
    print(RC.report("the same tensors", r))
    assert r["scale"] > 1 and r["y32"] > 100


# ------------------------------------------------------------------------------------------------------------------------ activation
def test_pre_activation_sets():
    a, f = RC.all_bf16(), RC.finite_bf16()
    assert a.dtype == f.dtype == torch.bfloat16 and a.numel() == 65536 and f.numel() == 65280
    assert len(set(a.view(torch.int16).tolist())) == 65536 and bool(torch.isfinite(f.float()).all())
    af = a.float()
    assert int(torch.isnan(af).sum()) == 254 and int((af == float("inf")).sum()) == 1 and int((af == float("-inf")).sum()) == 1
    x = RC.fp32_extra(65536)
    assert x.dtype == torch.float32 and x.numel() == 65536 and bool(torch.isfinite(x).all()) and float(x.abs().max()) < 2.0 ** 7
    assert not bool((x.bfloat16().float() == x).any())
    assert int(((x >= -9) & (x <= -3)).sum()) >= 4096 and int((x.abs() < 2.0 ** -126).sum()) > 0 and int((x > 0).sum()) > 20000


@pytest.mark.parametrize("flush", [False, True], ids=["exact", "denormals-flushed"])
@pytest.mark.parametrize("act", RC.ACTS)
def test_activation_twins_pass_exhaustively(act, flush):
    x = RC.finite_bf16().float()
    y = RC.act_twin(act, x, flush=flush)
    r16 = RC.check_act(act, True, x, y.to(torch.bfloat16))["post"]
    print(f"act2<{act}> twin over all finite bf16: error / bound {r16:.3f}")
    assert r16 <= 1.0
    if act == "gelu":                                                                    # the bound's second term is not what saves it
        ref = RC.act_reference(act, x)
        tight = RC.BF16_EPS * ref.abs() + 2.0 ** -24 * x.double().abs() + 2.0 ** -126
        assert float(((y.to(torch.bfloat16).double() - ref).abs() / tight).max()) <= 1.0


@pytest.mark.parametrize("act", RC.ACTS)
def test_torch_fp32_of_the_reference_activations_passes(act):
    fin, extra = RC.finite_bf16().float(), RC.fp32_extra(65536)
    if act == "gelu":
        # F.gelu overflows above 2^127 (module docstring of _rowop_cases); the float64 reference and the kernels' twin give x there
        top = fin[fin >= RC.TORCH_GELU_MAX]
        assert top.numel() == 128 and bool(torch.isinf(RC.act_torch(act, top)).all())
        assert RC.check_act(act, True, top, RC.act_twin(act, top).to(torch.bfloat16))["post"] <= 1.0
        fin = fin[fin < RC.TORCH_GELU_MAX]
    r16 = RC.act_torch_ratio(act, True, fin)["post"]
    r32 = max(RC.act_torch_ratio(act, False, fin)["post"], RC.act_torch_ratio(act, False, extra)["post"])
    print(f"torch fp32 {act}: error / bound  rounded to bf16 {r16:.3f}  fp32 {r32:.3f}")
    assert r16 <= 1.0 and r32 <= 1.0
    if act == "gelu":
        # the figure that moved the fp32 bound's second term from 2^-23 |x| to GELU_FP32_TAIL |x|
        ref = RC.act_reference(act, extra)
        err = (RC.act_torch(act, extra).double() - ref).abs()
        c = float(((err - 2.0 ** -21 * ref.abs() - 2.0 ** -126).clamp_min(0) / extra.double().abs()).max()) * 2.0 ** 23
        print(f"torch fp32 gelu needs {c:.2f} x 2^-23 |x| on fp32_extra (bound: {RC.GELU_FP32_TAIL * 2.0 ** 23:.2f})")
        assert c <= RC.GELU_FP32_TAIL * 2.0 ** 23
    # bf16 gelu: torch needs the bound's second term (it flushes the far tail to -0 and is many times over 2^-8 |ref| in (-5, -4])
    if act == "gelu":
        m = (fin > -5) & (fin <= -4)
        ref = RC.act_reference(act, fin[m])
        over = float(((RC.act_torch(act, fin[m]).bfloat16().double() - ref).abs() / (RC.BF16_EPS * ref.abs())).max())
        print(f"torch fp32 gelu rounded to bf16, (-5, -4]: {over:.1f} x (2^-8 |ref|)")
        assert over > 4 and bool((RC.act_torch(act, torch.tensor([-6.0, -8.0])) == 0).all())


def test_non_finite_pre_activations_as_the_reference_has_them():
    nan, inf = float("nan"), float("inf")
    x = torch.tensor([nan, inf, -inf])
    for act in RC.ACTS:
        y = RC.act_formula(act, x)
        assert math.isnan(float(y[0])) and float(y[1]) == inf
        assert (float(y[2]) == 0.0) if act == "relu" else math.isnan(float(y[2]))
        for bf16 in (True, False):
            assert RC.check_act(act, bf16, x, y)["post"] == 0.0
            for wrong in (torch.tensor([0.0, inf, y[2]]), torch.tensor([nan, nan, y[2]]), torch.tensor([nan, inf, -inf]),
                          torch.tensor([nan, inf, 1.0])):
                assert RC.check_act(act, bf16, x, wrong)["post"] == inf, (act, wrong)
    # all 65 536 patterns at once, as the stand-alone kernel gets them
    a = RC.all_bf16().float()
    for act in RC.ACTS:
        y = torch.where(torch.isfinite(a) & (a < RC.TORCH_GELU_MAX), RC.act_torch(act, a), RC.act_formula(act, a))
        y = torch.where(torch.isfinite(a) & (a >= RC.TORCH_GELU_MAX), a, y)
        assert RC.check_act(act, True, a, y.bfloat16())["post"] <= 1.0


@pytest.mark.parametrize("act,bug", [("gelu", "tanh_gelu"), ("gelu", "swapped"), ("quick_gelu", "swapped"), ("quick_gelu", "c17"),
                                     ("gelu", "zero_tail"), ("quick_gelu", "zero_tail"), ("gelu", "identity_head"),
                                     ("quick_gelu", "identity_head")])
def test_wrong_activation_twins_fail(act, bug):
    x = RC.finite_bf16().float()
    y = RC.act_twin(act, x, bug=bug)
    r16, r32 = RC.check_act(act, True, x, y.bfloat16())["post"], RC.check_act(act, False, x, y)["post"]
    print(f"{act} {bug}: error / bound  bf16 {r16:.3g}  fp32 {r32:.3g}")
    assert r32 > 1.0
    if (act, bug) == ("gelu", "identity_head"):
        # 1 - Phi(3) = 1.35e-3 is below 2^-9: x for gelu(x) above 3 is within ONE bf16 rounding of the truth, no bf16 bound can see it
        assert r16 <= 1.0
    else:
        assert r16 > 1.0


def test_the_older_assertions_accept_a_tanh_gelu_and_a_zeroed_tail():
    """test_native_vit_gpu's ``|post - gelu(pre)| < 5e-2`` and the ``2^-8 of the row's largest entry`` of test_gemm_mfma_shape_gpu /
    test_native_vit_gpu, on rows of N(0, 1) pre-activations: both accept a tanh-GELU and a tail zeroed below -3."""
    pre = torch.randn(64, 3072, generator=torch.Generator().manual_seed(3)).bfloat16().float()
    want = torch.nn.functional.gelu(pre)
    assert float(pre.min()) < -3.5
    for bug in ("tanh_gelu", "zero_tail"):
        post = RC.act_twin("gelu", pre, bug=bug).bfloat16().float()
        assert float((post - want).abs().max()) < 5e-2
        assert float(((post - want).abs().amax(dim=1) / want.abs().amax(dim=1)).max()) < 2.0 ** -8
        r = RC.check_act("gelu", True, pre, post.bfloat16())["post"]
        print(f"{bug} on N(0, 1) rows: accepted by both older assertions; error / bound here {r:.3g}")
        assert r > 10
    good = RC.act_twin("gelu", pre).bfloat16()
    assert RC.check_act("gelu", True, pre, good)["post"] <= 1.0


# ------------------------------------------------------------------------------------------------ token mean and L2 normalise
def _token_mean_twin(x, t0, skip_wave=None, divisor=None):
    """token_mean_kernel: wave w adds tokens t0 + w, t0 + w + 4, ... in fp32, ((p0 + p1) + p2) + p3, times 1 / (T - t0)"""
    x = x.numpy().astype(np.float32)
    B, T, d = x.shape
    part = np.zeros((4, B, d), np.float32)
    for wv in range(4):
        if wv != skip_wave:
            for t in range(t0 + wv, T, 4):
                part[wv] = part[wv] + x[:, t]
    inv = np.float32(1.0) / np.float32(divisor or (T - t0))
    return torch.from_numpy((((part[0] + part[1]) + part[2]) + part[3]) * inv)


@pytest.mark.parametrize("T,t0", [(17, 0), (17, 1), (2, 1), (1, 0), (2, 0), (4, 1)])
def test_token_mean_checker(T, t0):
    x = torch.randn(3, T, 264, generator=torch.Generator().manual_seed(T)).bfloat16().float()
    got = _token_mean_twin(x, t0)
    assert RC.check_token_mean(x, got, t0, False) <= 1.0 and RC.check_token_mean(x, got.bfloat16(), t0, True) <= 1.0
    assert RC.check_token_mean(x, x[:, t0:].mean(1), t0, False) <= 1.0
    if T - t0 >= 2:
        assert RC.check_token_mean(x, _token_mean_twin(x, t0, skip_wave=1).bfloat16(), t0, True) > 1.0      # a wave's tokens lost
        assert RC.check_token_mean(x, _token_mean_twin(x, t0, divisor=T - t0 + 1).bfloat16(), t0, True) > 1.0
    wrong = got.clone()
    wrong[1, 263] = 0.0                                                                  # one column of one image
    assert RC.check_token_mean(x, wrong.bfloat16(), t0, True) > 1.0


@pytest.mark.parametrize("n", [2, 16, 136, 1000])
def test_l2norm_checker(n):
    x = torch.randn(5, n, generator=torch.Generator().manual_seed(n)).bfloat16().float()
    x[3] = 0.0
    got = x / x.pow(2).sum(-1, keepdim=True).sqrt().clamp_min(1e-12)                     # torch fp32
    assert RC.check_l2norm(x, got, False) <= 1.0 and RC.check_l2norm(x, got.bfloat16(), True) <= 1.0
    assert bool((got[3] == 0).all())
    assert RC.check_l2norm(x, x / (x.pow(2).sum(-1, keepdim=True) + 1e-5 * n).sqrt(), False) > 1.0      # an eps under the root
    wrong = got.clone()
    wrong[4] = x[4] / x[:, : n - 1].pow(2).sum(-1).sqrt()[4]                             # the last element missing from the norm
    assert RC.check_l2norm(x, wrong, False) > 1.0
    wrong = got.clone()
    wrong[3, 0] = 1e-3                                                                   # the zero row must stay zero
    assert RC.check_l2norm(x, wrong, False) == float("inf")
    assert 6.0 <= RC.l2norm_units(n) <= 14.0
