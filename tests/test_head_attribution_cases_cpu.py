"""Direct logit attribution by head (vit_prisma_amd/logit_attribution.py) without a GPU: the planted cases of
tests/_attribution_cases.py are self-consistent, the PyTorch path of ``head_logit_attribution`` equals
``einsum(cache.stack_head_results(layer, apply_ln=True), answers)`` bit for bit on a small fp32 model (that helper is pinned to
the reference by tests/golden/cache_helpers_tiny.npz), the dispatcher says why it fell back, and ``pv_head_attribution`` refuses bad
arguments before it touches a device."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_vit_host_vs_golden import build
from vit_prisma_amd import _native, head_logit_attribution, logit_attribution
from vit_prisma_amd.synth import synth_images

import _attribution_cases as AC


@pytest.fixture(autouse=True)
def auto_mode():
    logit_attribution.use_native(None)
    yield
    logit_attribution.use_native(None)


@pytest.mark.parametrize("per_image", [False, True], ids=["shared", "per-image"])
@pytest.mark.parametrize("shape", AC.SHAPES, ids=AC.shape_id)
def test_cases_are_self_consistent(shape, per_image):
    case = AC.make_case(shape, per_image)
    B, T, L, H, dh, d, O = shape
    assert case.truth.shape == case.bound.shape == (B, T, L * H, O)
    # bf16-representable operands, answers that are not
    for a in (case.z, case.W_O):
        fin = np.isfinite(a)
        assert np.array_equal(AC.bf16(a[fin]), a[fin])
    assert (AC.bf16(case.answers) != case.answers).mean() > 0.9
    assert (case.scale > 0).all()
    # NaN exactly in the planted heads; each has a finite head beside it in the same row
    assert np.isnan(case.truth[case.nan]).all() and np.isfinite(case.truth[~case.nan]).all()
    assert np.isfinite(case.bound).all()
    rows = case.nan.any(axis=-1)
    assert rows[:, AC.TOK_NAN].all() and rows[:, AC.TOK_INF].all() and rows.sum() == 2 * B
    per_row = case.nan.reshape(B, T, L, H)[rows]
    assert (per_row.sum(axis=-1) == 1).all(), "one non-finite head per (row, layer): its neighbours are finite"
    # the zero head: exactly 0, with a bound of 0
    assert case.zero.any() and (case.truth[case.zero] == 0).all() and (case.bound[case.zero] == 0).all()
    live = ~case.nan & ~case.zero
    assert (case.bound[live] > 0).all()
    # centring matters: the uncentred form is further than twice the bound from the truth in most elements (the distance,
    # mean(a) sum_k r_k, is a zero-mean random number per element: some land near zero)
    off = np.abs(AC.uncentred(case)[live] - case.truth[live]) > 2 * case.bound[live]
    assert off.mean() > 0.8, off.mean()
    # layers are told apart: the same head of two layers differs by more than the two bounds, twice over
    t, b = case.truth.reshape(B, T, L, H, O), case.bound.reshape(B, T, L, H, O)
    keep = live.reshape(B, T, L, H)
    for l in range(1, L):
        both = keep[:, :, 0] & keep[:, :, l]
        apart = np.abs(t[:, :, 0] - t[:, :, l])[both] > 2 * (b[:, :, 0] + b[:, :, l])[both]
        assert apart.mean() > 0.8, (l, apart.mean())
    if per_image:
        # image 1 is the exact negative of image 0, and far enough from it that the wrong image's answers would show
        assert np.array_equal(case.truth[1][~case.nan[1]], -case.truth[0][~case.nan[0]])
        far = np.abs(case.truth[1] - case.truth[0])[live[0]] > 2 * (case.bound[0] + case.bound[1])[live[0]]
        assert far.mean() > 0.8, far.mean()
    else:
        # images are told apart
        far = np.abs(case.truth[1] - case.truth[0])[live[0] & live[1]] > 2 * (case.bound[0] + case.bound[1])[live[0] & live[1]]
        assert far.mean() > 0.8, far.mean()
    # the outlier head's bound is its own: before the division by the row's scale, larger than that of the plain row above it
    c = AC.HEAD_OUTLIER
    assert (case.bound[0, AC.TOK_OUTLIER, c] * case.scale[0, AC.TOK_OUTLIER] > 1.5 * case.bound[0, 0, c] * case.scale[0, 0]).all()


@pytest.fixture(scope="module")
def tiny():
    model, arch = build("tiny")
    with torch.no_grad():
        _, cache = model.run_with_cache(torch.from_numpy(synth_images(arch, 2, 1)))
    return model, cache


def _answers(model, per_image: bool, n_images: int) -> torch.Tensor:
    gen = torch.Generator().manual_seed(3)
    d = model.cfg.d_model
    shape = (n_images, 5, d) if per_image else (5, d)
    return 0.05 * torch.randn(*shape, generator=gen) + 0.02


@pytest.mark.parametrize("per_image", [False, True], ids=["shared", "per-image"])
@pytest.mark.parametrize("pos", [None, 0])
@pytest.mark.parametrize("layer", ["one", "all"])
def test_pytorch_path_equals_the_helpers_composition(tiny, layer, pos, per_image):
    model, cache = tiny
    n_layers, H = model.cfg.n_layers, model.cfg.n_heads
    layer = 1 if layer == "one" else n_layers
    answers = _answers(model, per_image, 2)
    with torch.no_grad():
        got, labels = head_logit_attribution(cache, answers, layer=layer, pos=pos)
        assert not logit_attribution.last_run_native
        stack, want_labels = cache.stack_head_results(layer, apply_ln=True, return_labels=True,
                                                      pos_slice=None if pos is None else [pos])
        want = torch.einsum("cbtd,bod->cbto" if per_image else "cbtd,od->cbto", stack, answers).permute(1, 2, 0, 3)
    assert labels == want_labels == [f"L{l}H{h}" for l in range(layer) for h in range(H)]
    T = cache["ln_final.hook_scale"].shape[1]
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, T if pos is None else 1, layer * H, 5)
    assert torch.equal(got, want)
    # None, -1 and n_layers name the same call
    if layer == n_layers and pos is None and not per_image:
        with torch.no_grad():
            for alias in (None, -1):
                assert torch.equal(head_logit_attribution(cache, answers, layer=alias, return_labels=False), want)


def test_dispatcher_reports_why_it_fell_back(tiny):
    model, cache = tiny
    answers = _answers(model, False, 2)
    with torch.no_grad():
        head_logit_attribution(cache, answers)
    assert not logit_attribution.last_run_native and "bf16" in logit_attribution.native_fallback_reason      # an fp32 model
    # a bf16 model whose cache sits on the CPU
    model16, arch = build("tiny")
    model16 = model16.to(torch.bfloat16)
    model16.cfg.dtype = torch.bfloat16
    with torch.no_grad():
        _, cache16 = model16.run_with_cache(torch.from_numpy(synth_images(arch, 2, 1)).to(torch.bfloat16))
        attr, labels = head_logit_attribution(cache16, answers, pos=0)
    assert not logit_attribution.last_run_native and "not on a GPU" in logit_attribution.native_fallback_reason
    assert attr.dtype == torch.float32 and tuple(attr.shape) == (2, 1, len(labels), 5)
    with torch.no_grad():
        head_logit_attribution(cache16, answers, layer=0)
    assert "layers below" in logit_attribution.native_fallback_reason
    logit_attribution.use_native(True)
    with pytest.raises(_native.NativeError, match="not on a GPU"):
        head_logit_attribution(cache16, answers)
    with pytest.raises(_native.NativeError, match="bf16"):
        head_logit_attribution(cache, answers)
    logit_attribution.use_native(False)
    with torch.no_grad():
        head_logit_attribution(cache, answers)
    assert logit_attribution.native_fallback_reason == "native_mode == 'off'"
    logit_attribution.use_native(None)
    with pytest.raises(ValueError):
        head_logit_attribution(cache, answers[:, :-1])
    with pytest.raises(ValueError):
        head_logit_attribution(cache, _answers(model, True, 3))
    with pytest.raises(IndexError):
        head_logit_attribution(cache, answers, layer=model.cfg.n_layers + 1)


def test_refusals_state_their_rule():
    """pv_head_attribution checks its arguments before it touches the device."""
    lib = _native.lib()
    assert lib.pv_head_attribution_workspace_bytes(12, 12, 64, 512) >= 12 * 512 * 768 * 4
    one = C.c_void_p(256)                         # never dereferenced: every call below is refused first
    ptrs = (C.c_void_p * 65)(*[256] * 65)

    def call(dtype=_native.PV_DTYPE_BF16, n_layers=2, B=2, T=50, pos=-1, H=12, dh=64, d=768, O=4, per_image=0, ws_bytes=1 << 20):
        return lib.pv_head_attribution(dtype, ptrs, ptrs, n_layers, B, T, pos, H, dh, d, one, one, O, per_image, one, one, ws_bytes, None)

    assert call(dtype=_native.PV_DTYPE_F32) == 1 and "bf16" in _native.last_error()
    for dh in (48, 76, 136, 16):
        assert call(dh=dh) == 1 and "d_head" in _native.last_error()
    assert call(d=772) == 1 and "multiple of 8" in _native.last_error()
    assert call(n_layers=0) == 1 and call(n_layers=65) == 1 and "64" in _native.last_error()
    assert call(O=0) == 1 and call(O=17) == 1 and "16" in _native.last_error()
    assert call(pos=-2) == 1 and call(pos=50) == 1 and "pos" in _native.last_error()
    assert call(B=1 << 15, T=1 << 10, H=16, dh=64) == 1 and "4 GiB" in _native.last_error()
    assert call(ws_bytes=16) == 3 and "workspace" in _native.last_error()
    assert call(per_image=1, ws_bytes=2 * 2 * 4 * 768 * 4 - 1) == 3 and "workspace" in _native.last_error()
