"""The patch-level logit lens (vit_prisma_amd/logit_lens.py) without a GPU: its PyTorch path against what the reference's own
prisma_tools/logit_lens.py returned on the tiny model (tests/golden/gen_golden_logit_lens.py), the vectorised dictionary against a
literal per-cell loop, the ``vit_prisma`` alias, the dispatcher's fallback reasons and the refusals of ``pv_logit_lens``."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_fro
from test_vit_host_vs_golden import build
from vit_prisma_amd import _native, logit_lens
from vit_prisma_amd.synth import synth_images


@pytest.fixture(scope="module")
def tiny():
    model, arch = build("tiny")
    with torch.no_grad():
        _, cache = model.run_with_cache(torch.from_numpy(synth_images(arch, 2, 1)))
    return model, cache, np.load(os.path.join(GOLDEN, "logit_lens_tiny.npz"))


@pytest.fixture(autouse=True)
def auto_mode():
    logit_lens.use_native(None)
    yield
    logit_lens.use_native(None)


@pytest.mark.parametrize("incl_mid", [False, True])
def test_pytorch_path_matches_reference(tiny, incl_mid):
    model, cache, g = tiny
    tag = "mid" if incl_mid else "pre"
    answers = model.head.W_H.detach().T.contiguous()
    assert np.array_equal(answers.numpy(), g["answers"])
    with torch.no_grad():
        directions, labels = logit_lens.get_patch_logit_directions(cache, answers, incl_mid=incl_mid)
    assert not logit_lens.last_run_native
    assert labels == [str(s) for s in g[f"labels_{tag}"]]
    assert directions.dtype == torch.float32 and tuple(directions.shape) == g[f"directions_{tag}"].shape
    # (the tolerance tests/test_activation_cache_helpers_cpu.py holds apply_ln_to_stack to)
    assert rel_fro(directions.numpy(), g[f"directions_{tag}"]) < 1e-5
    b, r = int(g["batch_idx"]), int(g["rank_index"])
    table = logit_lens.get_patch_logit_dictionary((directions, labels), batch_idx=b, rank_label=r)
    T, S = directions.shape[1], directions.shape[2]
    assert sorted(table) == list(range(T)) and all(len(table[t]) == S for t in table)
    idx = np.array([[table[t][s][2] for s in range(S)] for t in range(T)])
    rank = np.array([[table[t][s][3] for s in range(S)] for t in range(T)])
    logit = np.array([[table[t][s][0] for s in range(S)] for t in range(T)])
    assert np.array_equal(idx, g[f"dict_index_{tag}"])
    assert np.array_equal(rank, g[f"dict_rank_{tag}"])
    assert rel_fro(logit, g[f"dict_logit_{tag}"]) < 1e-5
    # the cache-level forms say the same on the PyTorch path
    with torch.no_grad():
        top_idx, top_logit, top_rank, labels2 = logit_lens.patch_logit_top(cache, answers, incl_mid=incl_mid, rank_index=r)
        table2 = logit_lens.patch_logit_dictionary(cache, answers, batch_idx=b, incl_mid=incl_mid, rank_label=r)
    assert labels2 == labels and tuple(top_idx.shape) == tuple(directions.shape[:3])
    assert np.array_equal(top_idx[b].numpy(), idx) and np.array_equal(top_rank[b].numpy(), rank)
    assert np.array_equal(top_logit[b].numpy(), logit.astype(np.float32))
    assert dict(table2) == dict(table)


def _literal_dictionary(directions, batch_idx, rank_index, class_names):
    """get_patch_logit_dictionary cell by cell (the reference's loop, with the tie rule of this package)."""
    out = {}
    for t, patches in enumerate(directions[batch_idx]):
        out[t] = []
        for logits in patches:
            vals = logits.tolist()
            best = max(range(len(vals)), key=lambda i: (vals[i], -i))
            name = str(best) if class_names is None else class_names[best]
            if rank_index is None:
                out[t].append((vals[best], name, best))
            else:
                lab = vals[rank_index]
                rank = sum(1 for i, v in enumerate(vals) if v > lab or (v == lab and i < rank_index))
                out[t].append((vals[best], name, best, rank))
    return out


def test_vectorised_dictionary_equals_the_literal_loop():
    gen = torch.Generator().manual_seed(7)
    B, T, S, O = 2, 6, 4, 37
    directions = torch.randn(B, T, S, O, generator=gen)
    # planted gaps: a clear winner in some cells, an exact tie between two columns in others (the lower index wins), and
    # columns equal to the label's logit on both sides of the label
    label = 11
    directions[0, :, 0, 20] = 9.0
    directions[0, :, 1, 30] = 7.5
    directions[0, :, 1, 4] = 7.5
    directions[0, :, 2, label] = 0.25
    directions[0, :, 2, 3] = 0.25
    directions[0, :, 2, 19] = 0.25
    directions[1] = directions[1].round()                  # many ties
    names = [f"class-{i}" for i in range(O)]
    for b in (0, 1):
        for rank_label, rank_index in ((None, None), (label, label), (names[label], label), (0, 0)):
            for class_names in (None, names):
                if isinstance(rank_label, str) and class_names is None:
                    with pytest.raises(ValueError):
                        logit_lens.get_patch_logit_dictionary(directions, b, rank_label)
                    continue
                got = logit_lens.get_patch_logit_dictionary(directions, b, rank_label, class_names)
                assert dict(got) == _literal_dictionary(directions, b, rank_index, class_names)
    # the tuple form reads its first entry
    assert dict(logit_lens.get_patch_logit_dictionary((directions, ["x"] * S), 1)) == _literal_dictionary(directions, 1, None, None)
    assert logit_lens.get_patch_logit_dictionary(directions, 0)[0][1][2] == 4                 # the tie went to the lower column
    assert logit_lens.get_patch_logit_dictionary(directions, 0, rank_label=label)[0][2][3] >= 1   # column 3 ties below the label


def test_alias_resolves_the_reference_import_path(tiny):
    import vit_prisma_amd
    from vit_prisma_amd import compat
    vit_prisma_amd.install_as("vit_prisma")
    try:
        from vit_prisma.prisma_tools.logit_lens import get_patch_logit_dictionary, get_patch_logit_directions
        assert get_patch_logit_directions is logit_lens.get_patch_logit_directions
        assert get_patch_logit_dictionary is logit_lens.get_patch_logit_dictionary
    finally:
        compat.uninstall("vit_prisma")
    assert vit_prisma_amd.logit_lens is logit_lens


def test_dispatcher_reports_why_it_fell_back(tiny):
    model, cache, _ = tiny
    answers = model.head.W_H.detach().T.contiguous()
    with torch.no_grad():
        logit_lens.get_patch_logit_directions(cache, answers)
    assert not logit_lens.last_run_native and "bf16" in logit_lens.native_fallback_reason     # an fp32 model
    # a bf16 model whose cache sits on the CPU
    model16, arch = build("tiny")
    model16 = model16.to(torch.bfloat16)
    model16.cfg.dtype = torch.bfloat16
    with torch.no_grad():
        _, cache16 = model16.run_with_cache(torch.from_numpy(synth_images(arch, 2, 1)).to(torch.bfloat16))
        top = logit_lens.patch_logit_top(cache16, answers.to(torch.bfloat16), rank_index=3)
    assert not logit_lens.last_run_native and "not on a GPU" in logit_lens.native_fallback_reason
    assert top[0].shape == (2, 17, 3) and top[2].shape == (2, 17, 3) and top[1].dtype == torch.float32
    logit_lens.use_native(True)
    with pytest.raises(_native.NativeError, match="not on a GPU"):
        logit_lens.get_patch_logit_directions(cache16, answers.to(torch.bfloat16))
    with pytest.raises(_native.NativeError, match="bf16"):
        logit_lens.patch_logit_top(cache, answers)
    logit_lens.use_native(False)
    with torch.no_grad():
        logit_lens.get_patch_logit_directions(cache, answers)
    assert logit_lens.native_fallback_reason == "native_mode == 'off'"


def test_refusals_state_their_rule():
    """pv_logit_lens checks its arguments before it touches the device."""
    lib = _native.lib()
    assert lib.pv_logit_lens_workspace_bytes(34, 5, 64, 24) >= 4 * (34 * 5 * 2 + 24 + 3 * 34 * 5)
    one = C.c_void_p(256)                         # never dereferenced: every call below is refused first
    taps = (C.c_void_p * 129)(*[256] * 129)

    def call(dtype=_native.PV_DTYPE_BF16, n_stack=1, d=64, directions=one, rank_of=-1, rank=None, ws_bytes=1 << 20):
        return lib.pv_logit_lens(dtype, taps, n_stack, 34, d, one, one, 24, directions, None, None, rank_of, rank, one, ws_bytes, None)

    assert call(dtype=_native.PV_DTYPE_F32) == 1 and "bf16" in _native.last_error()
    assert call(d=68) == 1 and "multiple of 8" in _native.last_error()
    assert call(n_stack=129) == 1 and "128" in _native.last_error()
    assert call(directions=None) == 1 and "no output" in _native.last_error()
    assert call(rank_of=24, rank=one) == 1 and "rank_of" in _native.last_error()
    assert call(ws_bytes=16) == 3 and "workspace" in _native.last_error()
