"""HookedTextTransformer on the HIP plan (pv_text_forward: token_embed_kernel, the blocks under attn_causal_kernel, eot_rows_kernel)
against the reference's own runs of ``synth.ARCHS["tiny-text"]`` (tests/golden/gen_golden_text.py).  Run with ``-m gpu`` on an MI355X.

fp32: keys, order, shapes, dtypes and -inf sets exact, rel-Frobenius < FP32_TOL over the finite entries and on the output.
bf16: each key's error against the fp32 fixture is held to the reference's OWN bf16 error for that key (text_tiny_bf16_budget.json)
times a margin -- see ``bf16_margin``; MEASURED.md has the table of measured ratios.  Measured on an MI355X: fp32 worst key 4.9e-7
(blocks.1.attn.hook_attn_scores), output 3.5e-7; bf16 ratios 0.81 .. 1.000 and one ``hook_scale`` key at 1.012.
"""
import pytest
import torch

from vit_prisma_amd.synth import ARCHS, synth_tokens

from _text_fixture import bf16_budget, text_tiny_full
from test_text_tower_cpu import BATCH, rel_fro, tiny_text_model

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4                   # the suite's (tests/test_native_vit_gpu.py)
BF16_SLACK = 1.0 + 1e-4           # "1.0 x" up to the norm's own rounding (tests/test_native_vit_gpu.py)
TINY_RATIO = 1.5                  # the suite's INTRA_BLOCK_RATIO: tiny models in bf16, where single roundings move the ratio
F32, BF16 = torch.float32, torch.bfloat16
ARCH = ARCHS["tiny-text"]
H, T = ARCH["n_heads"], ARCH["context_length"]

# bf16 margin over the reference's own bf16 error, per key.  Measured on the first GPU run (MEASURED.md, "Text tower, bf16: error
# against the reference's own"): 40 of the 41 keys and the output at 0.81 .. 1.0000 (the embedding keys and block 0's ln1 are the
# reference's bf16 tensors bit for bit), so they are held to 1.0 x BF16_SLACK.  The one key above 1 is blocks.0.ln2.hook_scale at
# 1.012: the suite's documented exception class (tests/test_native_vit_gpu.py) -- an fp32 per-token scalar sqrt(mean(x^2) + eps) of a
# bf16 residual stream, whose error IS the rounding noise of that stream (here resid_mid, the first tensor behind an accumulation the
# two implementations order differently), independent of the reference's and as large, so the ratio scatters around 1; over this
# fixture's 154 token rows it is held to the 1.15 x the suite asserts on its 200-row fixture (SCALE_SLACK_SMALL), well below the 1.5
# (INTRA_BLOCK_RATIO) it allows tiny models.  The other hook_scale keys measured below 1 and stay at 1.0 x.
SCALE_SLACK_SMALL = 1.15
LOOSE_BF16_KEYS = {"blocks.0.ln2.hook_scale": SCALE_SLACK_SMALL}
assert all(v <= TINY_RATIO for v in LOOSE_BF16_KEYS.values())


def bf16_margin(key: str) -> float:
    return LOOSE_BF16_KEYS.get(key, 1.0) * BF16_SLACK


def tokens_cuda():
    return torch.from_numpy(synth_tokens(ARCH, BATCH, seed=1)).cuda()


@pytest.fixture(scope="module")
def runs():
    """{dtype: (model, out, cache)} of the all-hooks native call, once per dtype"""
    got = {}
    for dtype in (F32, BF16):
        model = tiny_text_model(dtype, "cuda").use_native(True)
        with torch.no_grad():
            out, cache = model.run_with_cache(tokens_cuda())
        torch.cuda.synchronize()
        assert model.last_run_native, model.native_fallback_reason
        got[dtype] = (model, out, cache)
    return got


def test_fp32_against_the_reference(runs):
    G = text_tiny_full()
    model, out, cache = runs[F32]
    keys = [str(k) for k in G["__keys__"]]
    assert list(cache.keys()) == keys
    worst = ("", 0.0)
    for k in keys:
        got, want = cache[k].cpu(), torch.from_numpy(G[k])
        assert tuple(got.shape) == tuple(want.shape) and got.dtype == F32, k
        assert torch.equal(torch.isinf(got), torch.isinf(want)) and not torch.isnan(got).any(), k
        if k.endswith("hook_attn_scores"):
            assert int(torch.isinf(got).sum()) == BATCH * H * T * (T - 1) // 2 and bool((got[torch.isinf(got)] < 0).all()), k
        fin = torch.isfinite(want)
        r = rel_fro(got[fin], want[fin])
        worst = max(worst, (k, r), key=lambda t: t[1])
        assert r < FP32_TOL, (k, r)
    r = rel_fro(out.cpu(), torch.from_numpy(G["__out__"]))
    print(f"fp32 text tower: worst key {worst[0]} {worst[1]:.3g}, output {r:.3g}")
    assert out.dtype == F32 and tuple(out.shape) == G["__out__"].shape and r < FP32_TOL


def test_bf16_against_the_references_own_bf16_error(runs):
    G, budget = text_tiny_full(), bf16_budget()
    model, out, cache = runs[BF16]
    keys = [str(k) for k in G["__keys__"]]
    assert list(cache.keys()) == keys
    failed = []
    for k in keys + ["__out__"]:
        got = (out if k == "__out__" else cache[k]).cpu()
        want = torch.from_numpy(G[k])
        assert str(got.dtype).replace("torch.", "") == budget[k]["dtype"] and tuple(got.shape) == tuple(want.shape), k
        assert torch.equal(torch.isinf(got), torch.isinf(want)) and not torch.isnan(got).any(), k
        fin = torch.isfinite(want)
        err, ref_err = rel_fro(got.float()[fin], want[fin]), budget[k]["rel_fro"]
        ratio = err / ref_err if ref_err > 0 else (0.0 if err == 0 else float("inf"))
        print(f"bf16 text tower: {k:42s} err {err:.4g}  reference's own {ref_err:.4g}  ratio {ratio:.6f}  margin {bf16_margin(k):.4f}")
        if not err <= ref_err * bf16_margin(k):
            failed.append((k, ratio))
    assert not failed, failed


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_exact_keys(runs, dtype):
    model, out, cache = runs[dtype]
    tok = tokens_cuda()
    W, pos = model.token_embed.weight.detach(), model.pos_embed.detach()
    W_H, b_H = model.head.W_H.detach().float(), model.head.b_H.detach().float()
    assert torch.equal(cache["hook_embed"], W[tok])                                    # a pure gather
    assert torch.equal(cache["hook_full_embed"], (W[tok].float() + pos.float()).to(dtype))    # fp32 sum, one rounding
    assert torch.equal(cache["hook_pos_embed"], pos) and cache["hook_pos_embed"].shape == (T, ARCH["d_model"])
    assert torch.equal(cache["blocks.0.hook_resid_pre"], cache["hook_full_embed"])
    assert cache["blocks.0.hook_resid_pre"].data_ptr() == cache["hook_full_embed"].data_ptr()     # one buffer, as in the reference
    assert torch.equal(cache["blocks.1.hook_resid_pre"], cache["blocks.0.hook_resid_post"])
    above = torch.ones(T, T, dtype=torch.bool, device="cuda").triu(1).expand(BATCH, H, T, T)
    for l in range(ARCH["n_layers"]):
        assert bool(torch.isneginf(cache[f"blocks.{l}.attn.hook_attn_scores"][above]).all())
        assert bool((cache[f"blocks.{l}.attn.hook_pattern"][above] == 0).all())
    # the head reads the row at the FIRST maximal id: row 1 carries the EOT at 40 and again at 55
    eot = tok.argmax(dim=-1)
    assert eot.tolist() == [76, 40]
    pooled = cache["hook_ln_final"][torch.arange(BATCH, device="cuda"), eot]
    want = pooled.float() @ W_H + b_H
    got = cache["hook_post_head_pre_normalize"].float()
    tol = 2.0 ** -8 if dtype == BF16 else FP32_TOL
    assert rel_fro(got, want) < tol
    other = cache["hook_ln_final"][1, 55].float() @ W_H + b_H
    assert rel_fro(got[1], other) > 100 * tol                                          # (the second EOT's row is another one)
    assert rel_fro(out.float(), torch.nn.functional.normalize(got, dim=-1)) < tol


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_filtered_call_and_plain_forward_equal_the_all_hooks_call(runs, dtype):
    """Without an ln_final tap, ln_final runs on the B pooled rows only: the same output, bit for bit."""
    model, out, cache = runs[dtype]
    tok = tokens_cuda()
    with torch.no_grad():
        out2, c2 = model.run_with_cache(tok, names_filter=["hook_embed", "blocks.1.attn.hook_pattern", "hook_post_head_pre_normalize"])
        assert model.last_run_native, model.native_fallback_reason
        out3 = model(tok)
        assert model.last_run_native, model.native_fallback_reason
        out4, c4 = model.run_with_cache(tok.to(torch.int32), names_filter="blocks.0.hook_resid_pre", return_cache_object=False)
        assert model.last_run_native, model.native_fallback_reason
        _, c5 = model.run_with_cache(tok, names_filter="blocks.1.attn.hook_z", device="cpu", remove_batch_dim=False)
        assert model.last_run_native, model.native_fallback_reason
    assert list(c2.keys()) == ["hook_embed", "blocks.1.attn.hook_pattern", "hook_post_head_pre_normalize"]
    for k in c2.keys():
        assert torch.equal(c2[k], cache[k]), k
    assert torch.equal(out2, out) and torch.equal(out3, out) and torch.equal(out4, out)
    assert isinstance(c4, dict) and torch.equal(c4["blocks.0.hook_resid_pre"], cache["hook_full_embed"])
    assert c5["blocks.1.attn.hook_z"].device.type == "cpu" and torch.equal(c5["blocks.1.attn.hook_z"], cache["blocks.1.attn.hook_z"].cpu())


def test_an_id_outside_the_vocabulary_reads_nothing_and_gives_nan_rows(runs):
    model, _, cache = runs[F32]
    tok = tokens_cuda()
    tok[0, 3], tok[1, 9] = ARCH["vocab_size"], -1
    with torch.no_grad():
        _, c = model.run_with_cache(tok, names_filter=["hook_embed", "hook_full_embed"])
    assert model.last_run_native, model.native_fallback_reason
    bad = torch.zeros(BATCH, T, dtype=torch.bool, device="cuda")
    bad[0, 3] = bad[1, 9] = True
    for k in ("hook_embed", "hook_full_embed"):
        assert bool(torch.isnan(c[k][bad]).all()) and torch.equal(c[k][~bad], cache[k][~bad]), k


def test_fallback_reasons_are_distinct_and_the_pytorch_path_agrees(runs):
    model, out, cache = runs[F32]
    tok = tokens_cuda()
    model.use_native(None)
    seen = {}
    try:
        with torch.no_grad():
            out_h, _ = model.run_with_cache(tok, fwd_hooks=[("blocks.0.hook_resid_post", lambda t, hook: None)])
            seen["hooks"] = model.native_fallback_reason
            assert not model.last_run_native and rel_fro(out_h, out) < FP32_TOL
            with pytest.raises(RuntimeError):
                model.run_with_cache(tok[:, :40])
            seen["length"] = model.native_fallback_reason
            with pytest.raises(Exception):
                model.run_with_cache(tok.float())
            seen["dtype"] = model.native_fallback_reason
            cpu_model = tiny_text_model()
            cpu_model.run_with_cache(tok.cpu())
            seen["cpu"] = cpu_model.native_fallback_reason
        model.requires_grad_(True)
        model.run_with_cache(tok)
        seen["autograd"] = model.native_fallback_reason
        model.requires_grad_(False)
        keep = model.blocks[1]
        model.blocks[1] = tiny_text_model(F32, "cuda").blocks[1]
        with torch.no_grad():
            model.run_with_cache(tok)
        seen["tree"] = model.native_fallback_reason
        model.blocks[1] = keep
        with torch.no_grad():
            model.run_with_cache(tok)
        assert model.last_run_native, model.native_fallback_reason
    finally:
        model.requires_grad_(False)
        model.use_native(True)
    assert all(seen.values()) and len(set(seen.values())) == len(seen), seen
    assert "hook" in seen["hooks"] and "context_length" in seen["length"] and "integers" in seen["dtype"]
    assert "GPU" in seen["cpu"] and "autograd" in seen["autograd"] and "module tree" in seen["tree"]


def test_weight_edits_are_seen_and_freezing_skips_the_check(runs):
    model, out, _ = runs[F32]
    tok = tokens_cuda()
    nv = model._native
    with torch.no_grad():
        n0 = nv.n_repack
        model(tok)
        assert nv.n_repack == n0                                       # nothing changed: no repack
        saved = model.head.b_H.clone()
        model.head.b_H.add_(1.0)
        out2 = model(tok)
        assert nv.n_repack == n0 + 1 and not torch.equal(out2, out)
        model.head.b_H.copy_(saved)
        assert torch.equal(model(tok), out)
