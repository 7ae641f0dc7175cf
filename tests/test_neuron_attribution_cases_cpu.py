"""Direct logit attribution by MLP neuron (vit_prisma_amd/logit_attribution.py) without a GPU: the planted cases of
tests/_neuron_attribution_cases.py are self-consistent, the PyTorch path of ``neuron_logit_attribution`` equals
``einsum(cache.stack_neuron_results(layer, apply_ln=True), answers)`` bit for bit on a small fp32 model (that helper is pinned to the
reference by tests/golden/cache_helpers_tiny.npz; the path's neuron chunks are forced small here, so the chunking is exercised),
its top-k equals the oracle applied to that dense result, the dispatcher says why it fell back, and the two C entry points refuse
bad arguments before they touch a device."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_vit_host_vs_golden import build
from vit_prisma_amd import _native, logit_attribution, neuron_logit_attribution, top_neuron_logit_attribution
from vit_prisma_amd.synth import synth_images

import _neuron_attribution_cases as NC


@pytest.fixture(autouse=True)
def auto_mode():
    logit_attribution.use_native(None)
    yield
    logit_attribution.use_native(None)


@pytest.mark.parametrize("per_image", [False, True], ids=["shared", "per-image"])
@pytest.mark.parametrize("shape", NC.SHAPES, ids=NC.shape_id)
def test_cases_are_self_consistent(shape, per_image):
    case = NC.make_case(shape, per_image)
    B, T, L, M, d, O = shape
    assert case.truth.shape == case.bound.shape == (B, T, L * M, O)
    # bf16-representable operands, answers that are not
    for a in (case.post, case.W_out):
        fin = np.isfinite(a)
        assert np.array_equal(NC.bf16(a[fin]), a[fin])
    assert (NC.bf16(case.answers) != case.answers).mean() > 0.9
    assert (case.scale > 0).all()
    # NaN exactly at the planted neurons: one NaN and one +inf per image, on one token
    assert np.isnan(case.truth[case.nan]).all() and np.isfinite(case.truth[~case.nan]).all()
    assert np.isfinite(case.bound).all()
    assert case.nan.sum() == 2 * B and case.nan[:, NC.TOK_NONFINITE].sum() == 2 * B
    (ln, nn), (li, ni) = NC.nonfinite_neurons(L, M)
    assert np.isnan(case.post[ln, 0, NC.TOK_NONFINITE, nn]) and np.isposinf(case.post[li, 0, NC.TOK_NONFINITE, ni])
    assert L == 1 or ln != li, "the NaN and the infinity lie in different layers"
    # zeros: exact, with a bound of 0; the sparse token holds L M - 5 of them
    assert (case.truth[case.zero] == 0).all() and (case.bound[case.zero] == 0).all()
    assert (case.zero[:, NC.TOK_SPARSE].sum(axis=-1) == L * M - 5).all()
    live = ~case.nan & ~case.zero
    assert (case.bound[live] > 0).all()
    # centring matters: the uncentred form is further than twice the bound from the truth in most elements
    off = np.abs(NC.uncentred(case)[live] - case.truth[live]) > 2 * case.bound[live]
    assert off.mean() > 0.8, off.mean()
    # layers are told apart: the same neuron of two layers differs by more than the two bounds, twice over
    t, b = case.truth.reshape(B, T, L, M, O), case.bound.reshape(B, T, L, M, O)
    keep = live.reshape(B, T, L, M)
    for l in range(1, L):
        both = keep[:, :, 0] & keep[:, :, l]
        apart = np.abs(t[:, :, 0] - t[:, :, l])[both] > 2 * (b[:, :, 0] + b[:, :, l])[both]
        assert apart.mean() > 0.8, (l, apart.mean())
    if per_image:
        # image 1 is the exact negative of image 0, and far enough from it that the wrong image's answers would show
        assert np.array_equal(case.truth[1][~case.nan[1]], -case.truth[0][~case.nan[0]])
        far = np.abs(case.truth[1] - case.truth[0])[live[0]] > 2 * (case.bound[0] + case.bound[1])[live[0]]
    else:
        far = np.abs(case.truth[1] - case.truth[0])[live[0] & live[1]] > 2 * (case.bound[0] + case.bound[1])[live[0] & live[1]]
    assert far.mean() > 0.8, far.mean()
    # the outlier neurons' bound is their own: before the division by the row's scale, larger than that of the plain row above
    c = 1
    assert (case.bound[0, NC.TOK_OUTLIER, c] * case.scale[0, NC.TOK_OUTLIER] > 1.5 * case.bound[0, 0, c] * case.scale[0, 0]).all()
    # the tie token: four equal truths, the row's largest in magnitude in every column and the largest in value unless the answers
    # are the negated ones; the k-th largest of the oracle therefore lies inside the tie for k = 2 and k = 3
    flat = [l * M + n for l, n in NC.tie_neurons(L, M)]
    assert flat == sorted(flat) and len(set(flat)) == 4
    row = case.truth[:, NC.TOK_TIE]                                                    # [B, L M, O]
    others = np.delete(row, flat, axis=1)
    for f in flat[1:]:
        assert np.array_equal(row[:, f], row[:, flat[0]])
    # (with answers per image the planted row follows image 0's, which image 1 negates; a third image has answers of its own)
    images, both_signs = ([0], [0, 1]) if per_image else (range(B), range(B))
    assert all((np.abs(row[i, flat[0]]) > 1.5 * np.abs(others[i]).max(axis=0)).all() for i in both_signs)
    assert all((row[i, flat[0]] > 0).all() for i in images)
    for by in (0, 1):
        order = NC.topk_order(row.astype(np.float32), 3, by)                           # [B, O, 3]
        for i in (both_signs if by else images):
            assert (order[i] == np.array(flat[:3])).all(), "ties go to the lowest flat index"
    # the sparse token: three positive and two negative values in column 0 of image 0, everything else +-0
    sp = case.truth[0, NC.TOK_SPARSE, :, 0]
    assert (sp > 0).sum() == 3 and (sp < 0).sum() == 2
    # the oracle on the non-finite token: the NaN entries first, in index order, then the rest by key
    nf = NC.topk_order(case.truth[:, NC.TOK_NONFINITE].astype(np.float32), 3, 1)
    assert (nf[..., :2] == np.array(sorted([ln * M + nn, li * M + ni]))).all()


def test_shapes_reach_every_path_of_the_topk_kernel():
    """a mass tie above the candidate capacity exists (the radix-select path), and a row below it (the ranked path alone)"""
    sizes = [s[2] * s[3] for s in NC.SHAPES]
    assert min(sizes) <= NC.TOPK_CAP < sorted(sizes)[1], sizes
    assert min(sizes) < 256, "k = L M is tested on the smallest shape, inside PV_NATTR_MAX_K"
    assert any(s[2] * s[3] // 8 < 256 for s in NC.SHAPES) and any(s[2] * s[3] // 8 % 256 for s in NC.SHAPES)


def test_oracle_order():
    v = np.array([0.0, -0.0, 2.0, np.nan, -3.0, 2.0, np.inf, np.nan, -0.0], np.float32)[:, None]
    assert NC.topk_order(v, 9, 0)[0].tolist() == [3, 7, 6, 2, 5, 0, 1, 8, 4]
    assert NC.topk_order(v, 9, 1)[0].tolist() == [3, 7, 6, 4, 2, 5, 0, 1, 8]
    got = logit_attribution.topk_order(torch.from_numpy(v), 9, "value")[1][0].tolist()
    assert got == [3, 7, 6, 2, 5, 0, 1, 8, 4]
    assert logit_attribution.topk_order(torch.from_numpy(v), 9, "abs")[1][0].tolist() == [3, 7, 6, 4, 2, 5, 0, 1, 8]


def test_folded_truth_equals_the_reference_composition():
    """on the smallest shape, the literal composition in float64 agrees with the folded truth to 1e-12 relative"""
    for per_image in (False, True):
        case = NC.make_case(NC.SHAPES[0], per_image)
        ref = NC.reference_composition(case)
        ok = ~case.nan
        assert np.isnan(ref[case.nan]).all()
        scale = np.abs(case.truth[ok]).max()
        assert np.abs(ref[ok] - case.truth[ok]).max() <= 1e-12 * scale


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


@pytest.fixture
def small_slabs(tiny, monkeypatch):
    """neuron chunks of 48 on the tiny model's all-token calls (d_mlp = 128: chunks of 48, 48, 32)"""
    model, cache = tiny
    rows = cache["ln_final.hook_scale"].numel()
    assert model.cfg.d_mlp == 128
    monkeypatch.setattr(logit_attribution, "NEURON_SLAB_BYTES", 48 * rows * model.cfg.d_model * 4)


@pytest.mark.parametrize("per_image", [False, True], ids=["shared", "per-image"])
@pytest.mark.parametrize("pos", [None, 0])
@pytest.mark.parametrize("layer", ["one", "all"])
def test_pytorch_path_equals_the_helpers_composition(tiny, small_slabs, layer, pos, per_image):
    """Bit for bit: every element goes through the helpers' own operations (the product, the mean over d_model, the subtraction, the
    division), and the product with the answers sums over d_model alone, so that chunking over neurons changes no sum."""
    model, cache = tiny
    n_layers, M = model.cfg.n_layers, model.cfg.d_mlp
    layer = 1 if layer == "one" else n_layers
    answers = _answers(model, per_image, 2)
    with torch.no_grad():
        got, labels = neuron_logit_attribution(cache, answers, layer=layer, pos=pos)
        assert not logit_attribution.last_run_native
        stack, want_labels = cache.stack_neuron_results(layer, apply_ln=True, return_labels=True,
                                                        pos_slice=None if pos is None else [pos])
        want = torch.einsum("cbtd,bod->cbto" if per_image else "cbtd,od->cbto", stack, answers).permute(1, 2, 0, 3)
    assert labels == want_labels == [f"L{l}N{n}" for l in range(layer) for n in range(M)]
    T = cache["ln_final.hook_scale"].shape[1]
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, T if pos is None else 1, layer * M, 5)
    assert torch.equal(got, want)
    # the top-k of the same call: the oracle applied to the dense result
    for by, k in (("value", 7), ("abs", 1), ("abs", layer * M)):
        with torch.no_grad():
            top = top_neuron_logit_attribution(cache, answers, k, layer=layer, pos=pos, by=by)
        assert not logit_attribution.last_run_native
        order = NC.topk_order(want.numpy(), k, int(by == "abs"))
        assert tuple(top.values.shape) == tuple(top.layer.shape) == tuple(top.neuron.shape) == order.shape
        assert np.array_equal((top.layer * M + top.neuron).numpy(), order)
        assert torch.equal(top.values, torch.gather(want.movedim(-2, -1), -1, torch.from_numpy(order)))
    # None, -1 and n_layers name the same call
    if layer == n_layers and pos is None and not per_image:
        with torch.no_grad():
            for alias in (None, -1):
                assert torch.equal(neuron_logit_attribution(cache, answers, layer=alias, return_labels=False), want)


def test_dispatcher_reports_why_it_fell_back(tiny):
    model, cache = tiny
    answers = _answers(model, False, 2)
    with torch.no_grad():
        neuron_logit_attribution(cache, answers)
    assert not logit_attribution.last_run_native and "bf16" in logit_attribution.native_fallback_reason      # an fp32 model
    with torch.no_grad():
        top_neuron_logit_attribution(cache, answers, 4)
    assert not logit_attribution.last_run_native and "bf16" in logit_attribution.native_fallback_reason
    # a bf16 model whose cache sits on the CPU
    model16, arch = build("tiny")
    model16 = model16.to(torch.bfloat16)
    model16.cfg.dtype = torch.bfloat16
    with torch.no_grad():
        _, cache16 = model16.run_with_cache(torch.from_numpy(synth_images(arch, 2, 1)).to(torch.bfloat16))
        attr, labels = neuron_logit_attribution(cache16, answers, pos=0)
    assert not logit_attribution.last_run_native and "not on a GPU" in logit_attribution.native_fallback_reason
    assert attr.dtype == torch.float32 and tuple(attr.shape) == (2, 1, len(labels), 5)
    with torch.no_grad():
        empty = neuron_logit_attribution(cache16, answers, layer=0, return_labels=False)
    assert "layers below" in logit_attribution.native_fallback_reason and empty.shape[-2] == 0
    logit_attribution.use_native(True)
    with pytest.raises(_native.NativeError, match="not on a GPU"):
        neuron_logit_attribution(cache16, answers)
    with pytest.raises(_native.NativeError, match="not on a GPU"):
        top_neuron_logit_attribution(cache16, answers, 3)
    with pytest.raises(_native.NativeError, match="bf16"):
        neuron_logit_attribution(cache, answers)
    logit_attribution.use_native(False)
    with torch.no_grad():
        neuron_logit_attribution(cache, answers)
    assert logit_attribution.native_fallback_reason == "native_mode == 'off'"
    logit_attribution.use_native(None)
    M, n_layers = model.cfg.d_mlp, model.cfg.n_layers
    with pytest.raises(ValueError):
        neuron_logit_attribution(cache, answers[:, :-1])
    with pytest.raises(ValueError):
        neuron_logit_attribution(cache, _answers(model, True, 3))
    with pytest.raises(ValueError):
        top_neuron_logit_attribution(cache, answers[:, :-1], 3)
    with pytest.raises(ValueError):
        top_neuron_logit_attribution(cache, answers, 0)
    with pytest.raises(ValueError):
        top_neuron_logit_attribution(cache, answers, n_layers * M + 1)
    with pytest.raises(ValueError):
        top_neuron_logit_attribution(cache, answers, M + 1, layer=1)
    with pytest.raises(ValueError):
        top_neuron_logit_attribution(cache, answers, 3, by="magnitude")
    with pytest.raises(IndexError):
        neuron_logit_attribution(cache, answers, layer=n_layers + 1)


def test_refusals_state_their_rule():
    """pv_neuron_attribution and pv_neuron_attribution_topk check their arguments before they touch the device."""
    lib = _native.lib()
    assert lib.pv_neuron_attribution_workspace_bytes(12, 3072, 512) >= 12 * 512 * 3072 * 4
    assert lib.pv_neuron_attribution_workspace_bytes(0, 3072, 1) == 0
    good = dict(dtype=_native.PV_DTYPE_BF16, n_layers=2, B=2, T=50, pos=-1, M=3072, d=768, O=4, per_image=0, ws_bytes=1 << 20,
                k=16, by=0, ptrs=256, scale=256, answers=256, out=256, idx=256, ws=256)

    def call(topk, **kw):
        a = {**good, **kw}                         # (no pointer is ever dereferenced: every call below is refused first)
        ptrs = None if a["ptrs"] is None else (C.c_void_p * 65)(*[a["ptrs"]] * 65)
        head = (a["dtype"], ptrs, ptrs, a["n_layers"], a["B"], a["T"], a["pos"], a["M"], a["d"], a["scale"], a["answers"], a["O"],
                a["per_image"])
        if topk:
            return lib.pv_neuron_attribution_topk(*head, a["k"], a["by"], a["out"], a["idx"], a["ws"], a["ws_bytes"], None)
        return lib.pv_neuron_attribution(*head, a["out"], a["ws"], a["ws_bytes"], None)

    for topk in (False, True):
        def refused(text, code=1, **kw):
            assert call(topk, **kw) == code, kw
            assert text in _native.last_error(), (kw, _native.last_error())
            assert ("top-k" in _native.last_error()) == topk

        refused("bf16", dtype=_native.PV_DTYPE_F32)
        for M in (3076, 4, 0):
            refused("d_mlp", M=M)
        refused("multiple of 8", d=772)
        refused("64", n_layers=0)
        refused("64", n_layers=65)
        refused("16", O=0)
        refused("16", O=17)
        refused("pos", pos=-2)
        refused("pos", pos=50)
        refused("4 GiB", B=1 << 10, T=1 << 10, M=2048)
        for name in ("ptrs", "scale", "answers", "ws"):
            refused("NULL", **{name: None})
        refused("val and idx must be" if topk else "out must be", out=None)
        refused("aligned", answers=260)
        refused("aligned", ws=264)
        refused("aligned", ptrs=258)
        refused("aligned", scale=258)
        refused("aligned", out=258)
        refused("workspace", code=3, ws_bytes=16)
        refused("workspace", code=3, per_image=1, ws_bytes=2 * 2 * 4 * 3072 * 4 - 1)
    assert call(True, k=0) == 1 and "PV_NATTR_MAX_K" in _native.last_error()
    assert call(True, k=257) == 1 and "256" in _native.last_error()
    assert call(True, k=41, n_layers=1, M=40) == 1 and "n_layers * d_mlp" in _native.last_error()
    assert call(True, by=2) == 1 and call(True, by=-1) == 1 and "by must be" in _native.last_error()
    assert call(True, idx=None) == 1 and "idx" in _native.last_error()
    assert call(True, idx=258) == 1 and "aligned" in _native.last_error()
