"""The dense SAE steps of csrc/sae_dense.hip and csrc/sae_gated.hip (the GEMM: csrc/sae_dense_gemm.hip) on planted operand ranges
(tests/_sae_dense_cases.py): ``dense_step`` and ``gated_step`` through NativeSAE, in the split-fp16 form and in the exact fp32 form
(forced through the tuning key dense_fp32, or taken by the kernels on their own at N % 4 != 0).  Every element of the reconstruction, of dH (left in the workspace), of every gradient tensor and the scalars are held
to a bound derived from the float64 reference's own absolute sums and the stated rounding model (no tensor-wide norm, nothing fitted);
gates, firing counts and l0 exactly; ``exact_grid`` and ``no_firing`` add their exact assertions, ``shrinking`` the bit-identity with a fresh
engine.  The split form's tracked operand maxima are read back and must be the tensors' own.  Every test prints its worst error / bound
ratios (MEASURED.md: "dense split-fp16 form, planted cases")."""
import functools

import numpy as np
import pytest
import torch

import _sae_dense_cases as DC
from vit_prisma_amd.sae.native_sae import NativeSAE

pytestmark = pytest.mark.gpu
AM_X, AM_WENC, AM_F, AM_WDEC, AM_DY, AM_DH = range(6)                           # dense_step_body's slot arrays of ws.dense_amax


@functools.lru_cache(maxsize=None)
def case_bounds(name, form):
    """one float64 reference and one set of bounds per case and form, shared by the tests (read-only)"""
    return DC.bounds(DC.case(name), form)


def engine(c, P=None):
    T = {k_: torch.from_numpy(np.ascontiguousarray(v).copy()).cuda() for k_, v in (P or c.P).items()}
    gated = {k_: T[k_] for k_ in ("b_gate", "r_mag", "b_mag")} if c.kind == "gated" else None
    return NativeSAE(T["W_enc"], T["W_dec"], T["b_enc"], T["b_dec"], 8, "none", c.n, gated=gated, activation=c.activation,
                     lp_norm=c.lp_norm)


def ws_region(eng, name, shape, dtype=torch.float32):
    off = eng.lib.pv_debug_sae_ws_offset(eng._plan, name)
    assert off != (1 << 64) - 1, name
    return eng.workspace[off:off + int(np.prod(shape)) * 4].view(dtype).view(*shape)


def step(eng, c, x, through_relu_step=False):
    xt = torch.from_numpy(np.array(x, np.float32)).cuda()
    if c.kind == "gated":
        eng.gated_step(xt, c.l1, want_out=True, sparse=False)
    elif through_relu_step:
        eng.relu_step(xt, c.l1, want_out=True, renorm_decoder=c.renorm)
    else:
        eng.dense_step(xt, c.l1, want_out=True, renorm_decoder=c.renorm)
    torch.cuda.synchronize()


def gathered(eng, c):
    """what the step left, as the checker takes it"""
    n, Fs = c.n, c.d_sae
    sc = eng.scalars.cpu().numpy()
    got = dict(loss=sc[0], mse=sc[1], l0=sc[2], l1=sc[4], sae_out=eng.sae_out[:n].cpu().numpy(), gW_dec=eng.g["W_dec"].cpu().numpy(),
               gW_enc=eng.g["W_enc"].cpu().numpy(), gb_dec=eng.g["b_dec"].cpu().numpy(), fire_count=eng.fire_count.cpu().numpy())
    if c.kind == "relu":
        got["gb_enc"] = eng.g["b_enc"].cpu().numpy()
        got["dH"] = ws_region(eng, b"hidden", (n, Fs)).cpu().numpy()
        got["gates"] = got["dH"] != 0
    else:
        hs = eng._gt_scratch[:2 * n * Fs * 4].view(torch.float32).view(2, n, Fs).cpu().numpy()      # gated_carve: hs comes first
        got.update(aux=sc[6], dP=hs[0], dG=hs[1], gb_gate=eng.g["b_gate"].cpu().numpy(), gb_mag=eng.g["b_mag"].cpu().numpy(),
                   gr_mag=eng.g["r_mag"].cpu().numpy())
    return got


def tracked_maxima_are_the_tensors_own(eng, c, got, label):
    """the three producers of the split form's operand maxima: dense_absmax3_kernel (sae_in, W_enc^T, W_dec), dense_finish_kernel (dY), the
    DH epilogue (dH); f's is gone with f.  A maximum over the 256 slots must be the bit pattern of the tensor's largest |entry|."""
    am = ws_region(eng, b"dense_amax", (16, DC.DG_AMAX_SLOTS), torch.int32).cpu().numpy().view(np.uint32)
    dY = ws_region(eng, b"dY", (c.n, c.d_in)).cpu().numpy()
    si = ws_region(eng, b"sae_in", (c.n, c.d_in)).cpu().numpy()
    want = {AM_X: si, AM_WENC: eng.W_encT.cpu().numpy(), AM_WDEC: eng.params["W_dec"].cpu().numpy(), AM_DY: dY, AM_DH: got["dH"]}
    for slot, t in want.items():
        m = np.abs(t).max().astype(np.float32)
        assert am[slot].max() == m.view(np.uint32), f"{label}: tracked maximum {slot}: {am[slot].max().view(np.float32)!r}, tensor {m!r}"
    assert np.array_equal(si, (c.x - c.P["b_dec"]).astype(np.float32)), f"{label}: sae_in"


def verdict(label, ratios, msgs):
    print(f"[dense-planted] {label}: {DC.fmt(ratios)}")
    assert DC.passes(ratios), f"{label}: " + "; ".join(msgs)


RELU_CASES = ("exact_grid", "ragged_random", "ragged_exact_form", "outlier", "no_firing", "tail")     # (+ shrinking, gated_gate_larger below)
assert set(RELU_CASES) | {"shrinking", "gated_gate_larger"} == set(DC.CASES)


@pytest.mark.parametrize("name", RELU_CASES)
def test_dense_step_on_planted_ranges(name, tuning):
    c = DC.case(name)
    gates = {}
    for form, fp32 in c.forms:
        if fp32 is not None:
            tuning("dense_fp32", fp32)
        label = f"dense_step {name} {form}" + ("" if fp32 is None else f" (dense_fp32={fp32})")
        eng = engine(c)
        eng.flat_g.fill_(float("nan"))
        w_dec_before = eng.params["W_dec"].clone()
        step(eng, c, c.x)
        got = gathered(eng, c)
        for q, v in got.items():
            assert np.isfinite(np.asarray(v, np.float64)).all(), f"{label}: {q} holds NaN or inf"
        ratios, msgs = DC.check(c, form, got, bnd=case_bounds(name, form))
        if name == "exact_grid":
            assert torch.equal(eng.params["W_dec"].view(torch.int32), w_dec_before.view(torch.int32)), f"{label}: the renorm moved W_dec"
        verdict(label, ratios, msgs)
        if form == "split" and c.n % 4 == 0:
            tracked_maxima_are_the_tensors_own(eng, c, got, label)
        gates[form] = got["gates"]
        if name in ("ragged_random", "outlier"):
            # relu_step: below 2048 features it has no sparse form, so the same five GEMMs run behind its device-side mode word
            # (every kernel's ``gate`` argument) -- the same bits, and mode 1
            other = engine(c)
            other.flat_g.fill_(float("nan"))
            step(other, c, c.x, through_relu_step=True)
            assert int(other.relu_mode.item()) == 1, label
            for a, b, what in ((other.flat_g, eng.flat_g, "gradients"), (other.sae_out, eng.sae_out, "sae_out"),
                               (other.scalars[:5], eng.scalars[:5], "scalars"), (other.fire_count, eng.fire_count, "fire_count")):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{label}: relu_step differs from dense_step in {what}"
        tuning("reset")
    if len(gates) == 2:
        assert np.array_equal(gates["split"], gates["exact"]), f"{name}: the two forms disagree on a gate"


def test_second_step_at_a_smaller_scale_equals_a_fresh_engine(tuning):
    """``shrinking``: a step on x 2^12, then one on x with no apply between them -- the second within its own bounds and, bit for bit, a fresh
    engine's step on x (operand maxima left over from the larger step would show in every GEMM)"""
    c = DC.case("shrinking")
    for form, fp32 in c.forms:
        if fp32 is not None:
            tuning("dense_fp32", fp32)
        used, fresh = engine(c), engine(c)
        for x in c.xs:
            step(used, c, x)
        step(fresh, c, c.x)
        got = gathered(used, c)
        got["fresh"] = gathered(fresh, c)
        ratios, msgs = DC.check(c, form, got, bnd=case_bounds("shrinking", form))
        verdict(f"dense_step shrinking {form}", ratios, msgs)
        assert torch.equal(used.flat_g.view(torch.int32), fresh.flat_g.view(torch.int32)), f"{form}: gradient bits"
        assert torch.equal(used.scalars.view(torch.int32), fresh.scalars.view(torch.int32)), f"{form}: scalars"
        tuning("reset")


def test_gated_step_with_the_gate_plane_larger(tuning):
    """``gated_gate_larger``: relu(gate) 2^12 and more above feature_acts on half of the tokens, the reverse on the others; the reference is
    built on the decoder rows as the step's renorm left them"""
    c = DC.case("gated_gate_larger")
    counts = {}
    for form, fp32 in c.forms:
        if fp32 is not None:
            tuning("dense_fp32", fp32)
        eng = engine(c)
        eng.flat_g.fill_(float("nan"))
        step(eng, c, c.x)
        got = gathered(eng, c)
        for q, v in got.items():
            assert np.isfinite(np.asarray(v, np.float64)).all(), f"gated_step {form}: {q} holds NaN or inf"
        P = dict(c.P, W_dec=eng.params["W_dec"].cpu().numpy())
        assert (eng.g["b_enc"] == 0).all()
        ratios, msgs = DC.check(c, form, got, P=P)
        verdict(f"gated_step gated_gate_larger {form}", ratios, msgs)
        counts[form] = (got["fire_count"], got["dG"] != 0)
        tuning("reset")
    assert np.array_equal(counts["split"][0], counts["exact"][0]) and np.array_equal(counts["split"][1], counts["exact"][1])
