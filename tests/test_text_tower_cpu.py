"""HookedTextTransformer without a GPU: the PyTorch path against the reference's own run, the state-dict surface, the open_clip
text converter, the text registry, the ``install_as`` aliases, what ``pv_text_plan_create`` accepts and refuses, and the tap planner's
order for a text model.

Fixtures (tests/golden/gen_golden_text.py, which executes the reference on the CPU):
* ``text_tiny_full.npz`` (+ parts)       the reference's fp32 run of ``synth.ARCHS["tiny-text"]`` on ``synth_tokens`` (batch 2; row 1
  carries the EOT twice): every cache tensor, the key order, the output, the ids;
* ``weight_conversion_text_tiny.npz``    a random open_clip text state dict and the reference converter's result;
* ``model_registry_text.json``           the fields of the registry's OPEN_CLIP_TEXT_CONFIGS.
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

from vit_prisma_amd import HookedTextTransformer, HookedTextTransformerConfig, _native
from vit_prisma_amd.synth import ARCHS, synth_text_state, synth_tokens

from _text_fixture import GOLDEN, text_tiny_full

TIGHT = 1e-5
BATCH = 2


def rel_fro(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def tiny_text_model(dtype=torch.float32, device="cpu", **kw) -> HookedTextTransformer:
    """``tiny-text`` from ``synth_text_state`` seed 0: the model of text_tiny_full.npz (shared with tests/test_text_tower_gpu.py)"""
    arch = ARCHS["tiny-text"]
    model = HookedTextTransformer(HookedTextTransformerConfig(**arch, dtype=dtype, device=device), **kw)
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(v) for k, v in synth_text_state(arch, seed=0).items()}, strict=False)
    assert sorted(missing) == ["ln_pre.b", "ln_pre.w"] and not unexpected
    return model.to(dtype).to(device).eval()


@pytest.fixture(scope="module")
def torch_run():
    model = tiny_text_model()
    tokens = torch.from_numpy(synth_tokens(ARCHS["tiny-text"], BATCH, seed=1))
    with torch.no_grad():
        out, cache = model.run_with_cache(tokens)
    return model, tokens, out, cache


def test_tokens_are_the_fixtures_and_plant_the_eot_twice():
    G = text_tiny_full()
    arch = ARCHS["tiny-text"]
    tok = synth_tokens(arch, BATCH, seed=1)
    assert np.array_equal(tok, G["__tokens__"]) and tok.dtype == np.int64
    eot = arch["vocab_size"] - 1
    assert tok.max() == eot and tok[0].argmax() == 76
    assert tok[1, 40] == eot and tok[1, 55] == eot and torch.from_numpy(tok)[1].argmax().item() == 40
    assert torch.tensor([3, 9, 9, 0]).argmax().item() == 1           # torch.argmax returns the first


def test_pytorch_path_keys_order_and_shapes_equal_the_reference(torch_run):
    G = text_tiny_full()
    _, _, out, cache = torch_run
    keys = [str(k) for k in G["__keys__"]]
    assert len(keys) == 41 and list(cache.keys()) == keys
    for k in keys:
        assert tuple(cache[k].shape) == G[k].shape, k
    assert cache["hook_pos_embed"].shape == (77, 128)                  # the parameter slice: no batch dimension
    assert tuple(out.shape) == G["__out__"].shape == (BATCH, 48)


def test_pytorch_path_values_and_inf_sets_equal_the_reference(torch_run):
    G = text_tiny_full()
    model, _, out, cache = torch_run
    assert not model.last_run_native and model.native_fallback_reason == "input is not on a GPU"
    H, T = 2, 77
    for k in (str(k) for k in G["__keys__"]):
        got, want = cache[k], torch.from_numpy(G[k])
        assert torch.equal(torch.isinf(got), torch.isinf(want)) and not torch.isnan(got).any(), k
        fin = torch.isfinite(want)
        assert rel_fro(got[fin], want[fin]) < TIGHT, k
        if k.endswith("hook_attn_scores"):
            assert int(torch.isinf(got).sum()) == BATCH * H * T * (T - 1) // 2, k
            assert (got[torch.isinf(got)] < 0).all(), k
            assert torch.equal(torch.isinf(got), torch.ones(T, T, dtype=torch.bool).triu(1).expand(BATCH, H, T, T)), k
        if k.endswith("hook_pattern"):
            assert (got[torch.ones(T, T, dtype=torch.bool).triu(1).expand(BATCH, H, T, T)] == 0).all(), k
    assert rel_fro(out, torch.from_numpy(G["__out__"])) < TIGHT


def test_state_dict_keys_are_the_references():
    model = tiny_text_model()
    per_block = ["ln1.w", "ln1.b", "attn.W_Q", "attn.W_K", "attn.W_V", "attn.W_O", "attn.b_Q", "attn.b_K", "attn.b_V", "attn.b_O",
                 "ln2.w", "ln2.b", "mlp.W_in", "mlp.b_in", "mlp.W_out", "mlp.b_out"]
    want = ["token_embed.weight", "pos_embed", "ln_pre.w", "ln_pre.b", "ln_final.w", "ln_final.b", "head.W_H", "head.b_H"]
    want += [f"blocks.{l}.{n}" for l in range(2) for n in per_block]
    assert sorted(model.state_dict()) == sorted(want)                  # attn_mask is a non-persistent buffer
    assert "attn_mask" in dict(model.named_buffers()) and model.attn_mask.shape == (77, 77)
    assert "hook_ln_pre" in model.hook_dict and "ln_pre.hook_scale" in model.hook_dict      # exist, never fire


def test_no_causal_mask_gives_no_inf_anywhere():
    model = tiny_text_model(no_causal_mask=True)
    assert model.attn_mask is None
    with torch.no_grad():
        _, cache = model.run_with_cache(torch.from_numpy(synth_tokens(ARCHS["tiny-text"], BATCH, seed=1)))
    for k, v in cache.items():
        assert torch.isfinite(v).all(), k
    assert (cache["blocks.0.attn.hook_pattern"][:, :, 0, 1:] > 0).all()     # the first query sees the future


def test_cls_token_raises_in_the_constructor():
    with pytest.raises(NotImplementedError):
        HookedTextTransformer(HookedTextTransformerConfig(**ARCHS["tiny-text"], device="cpu"), cls_token=True)


def test_a_short_prompt_raises_on_the_pytorch_path_like_the_reference():
    model = tiny_text_model()
    tokens = torch.from_numpy(synth_tokens(ARCHS["tiny-text"], BATCH, seed=1))[:, :40]
    with torch.no_grad(), pytest.raises(RuntimeError, match="size of tensor"):
        model(tokens)


def test_converter_equals_the_reference_bit_for_bit_and_loads():
    from vit_prisma_amd.weights import convert_open_clip_text_weights
    G = np.load(os.path.join(GOLDEN, "weight_conversion_text_tiny.npz"))
    dims = json.loads(str(G["__cfg__"]))
    cfg = HookedTextTransformerConfig(**{**ARCHS["tiny-text"], **dims}, device="cpu")
    old = {k[3:]: torch.from_numpy(G[k]) for k in G.files if k.startswith("in.")}
    new = convert_open_clip_text_weights(old, cfg)
    assert sorted(new) == sorted(str(k) for k in G["__out_keys__"])
    for k, v in new.items():
        want = G["out." + k]
        assert tuple(v.shape) == want.shape and v.dtype == torch.float32 and np.array_equal(v.numpy(), want), k
    model = HookedTextTransformer(cfg)
    missing, unexpected = model.load_state_dict(new, strict=False)
    assert sorted(missing) == ["ln_pre.b", "ln_pre.w"] and not unexpected


def test_text_registry_equals_the_reference_and_the_vision_tables_are_untouched():
    from vit_prisma_amd import model_loader as ML
    with open(os.path.join(GOLDEN, "model_registry_text.json")) as f:
        reg = json.load(f)
    assert sorted(reg) == ML.list_available_text_models() and len(reg) >= 14
    for name, fields in reg.items():
        cfg = ML.load_text_config(name, device="cpu")
        assert isinstance(cfg, HookedTextTransformerConfig) and cfg.model_name == name
        assert cfg.d_head == 64 and cfg.context_length == 77 and fields
        for k, v in fields.items():
            assert getattr(cfg, k) == v, (name, k, getattr(cfg, k), v)
    # what the vision entry points return is pinned elsewhere; here: the text names did not leak into them
    vision = ML.list_available_models()
    assert vision == sorted({**ML.MODEL_ARCH, **ML.DINO_ARCH, **ML.WIDE_ARCH}) and len(vision) == 13
    cfg = ML.load_config("open-clip:laion/CLIP-ViT-B-32-DataComp.XL-s13B-b90K", device="cpu")
    assert type(cfg).__name__ == "HookedViTConfig" and not hasattr(cfg, "context_length") and cfg.patch_size == 32
    with pytest.raises(ValueError):
        ML.load_config("open-clip:laion/CoCa-ViT-B-32-laion2B-s13B-b90k", device="cpu")


def test_install_as_serves_the_references_import_paths():
    import vit_prisma_amd
    from vit_prisma_amd import compat
    assert "vit_prisma" not in sys.modules or getattr(sys.modules["vit_prisma"], "_pv_alias", False)
    vit_prisma_amd.install_as("vit_prisma")
    try:
        from vit_prisma.configs.HookedTextTransformerConfig import HookedTextTransformerConfig as RefCfg
        from vit_prisma.models.base_text_transformer import HookedTextTransformer as RefCls
        assert RefCls is HookedTextTransformer and RefCfg is HookedTextTransformerConfig
        import vit_prisma
        assert vit_prisma.HookedTextTransformer is HookedTextTransformer
    finally:
        compat.uninstall("vit_prisma")


def _desc(**kw):
    base = dict(n_layers=12, d_model=512, n_heads=8, d_head=64, d_mlp=2048, context_length=77, vocab_size=49408, n_classes=512,
                has_head=1, normalize_output=1, causal=1, activation=0, dtype=1, eps=1e-5, attn_scale=8.0)
    base.update(kw)
    return _native.TextDesc(**base)


def test_text_plan_creation_accepts_clip_shapes_and_states_the_rule_when_it_refuses():
    lib = _native.lib()
    plan = C.c_void_p()
    for kw in (dict(), dict(d_model=768, n_heads=12, d_mlp=3072), dict(dtype=0), dict(causal=0, d_head=80, n_heads=8, d_model=640)):
        desc = _desc(**kw)
        assert lib.pv_text_plan_create(C.byref(desc), C.byref(plan)) == 0, (kw, _native.last_error())
        assert lib.pv_vit_shadow_bytes(plan) > 0 and lib.pv_vit_workspace_bytes(plan, 4) > 0
        lib.pv_vit_plan_destroy(plan)
    for kw, words in ((dict(context_length=2049), ("context_length", "2048")),
                      (dict(d_head=80, n_heads=8, d_model=640), ("causal", "{32, 64}")),
                      (dict(d_model=2056), ("d_model", "multiple of 8", "2048")),
                      (dict(d_model=516), ("d_model", "multiple of 8"))):
        desc = _desc(**kw)
        assert lib.pv_text_plan_create(C.byref(desc), C.byref(plan)) == 1, kw
        why = _native.last_error()
        assert all(w in why for w in words), (kw, why)


def test_forward_entries_refuse_the_other_kind_of_plan_before_any_launch():
    """No GPU here: a call that got as far as a launch would fail with a HIP error (status 2), not with PV_ERR_INVALID (1)."""
    lib = _native.lib()
    tplan, vplan = C.c_void_p(), C.c_void_p()
    desc = _desc(n_layers=1)
    assert lib.pv_text_plan_create(C.byref(desc), C.byref(tplan)) == 0
    vdesc = _native.VitDesc(n_layers=1, d_model=64, n_heads=2, d_head=32, d_mlp=128, n_channels=3, patch_size=8, image_size=32,
                            n_tokens=17, n_classes=24, use_cls_token=1, layer_norm_pre=1, has_head=1, normalize_output=1, activation=0,
                            dtype=0, eps=1e-5, attn_scale=32 ** 0.5, pooling=0)
    assert lib.pv_vit_plan_create(C.byref(vdesc), C.byref(vplan)) == 0
    buf = (C.c_char * 4096)()
    p = C.addressof(buf) // 256 * 256 + 256
    assert lib.pv_text_forward(vplan, p, 1, 1, None, 0, p, 1 << 30, p, None) == 1
    assert "pv_text_plan_create" in _native.last_error()
    assert lib.pv_vit_forward(tplan, p, 1, 1, 1, None, 0, p, 1 << 30, p, None) == 1
    lib.pv_vit_plan_destroy(tplan)
    lib.pv_vit_plan_destroy(vplan)


def test_pv_attention_refuses_causal_wide_heads_with_the_rule():
    lib = _native.lib()
    buf = (C.c_char * 4096)()
    p = C.addressof(buf) // 256 * 256 + 256
    assert lib.pv_attention(0, p, p, p, 1, 77, 2, 80, 80 ** 0.5, 1, None, None, p, None) == 1
    why = _native.last_error()
    assert "causal" in why and "{32, 64}" in why, why


def test_tap_plan_order_for_text_equals_the_fixture():
    from vit_prisma_amd.tap_plan import hook_order, tap_spec
    G = text_tiny_full()
    cfg = HookedTextTransformerConfig(**ARCHS["tiny-text"], device="cpu")
    assert hook_order(cfg, cfg.n_layers, True) == [str(k) for k in G["__keys__"]]
    cfg_pre = HookedTextTransformerConfig(**{**ARCHS["tiny-text"], "layer_norm_pre": True}, device="cpu")     # (the registry sets it)
    assert hook_order(cfg_pre, cfg.n_layers, True) == [str(k) for k in G["__keys__"]]
    S = _native.SLOT
    assert tap_spec("hook_embed", cfg, 2, 77).shape == (2, 77, 128)
    assert tap_spec("hook_pos_embed", cfg, 2, 77).shape == (77, 128)
    full, pre0 = tap_spec("hook_full_embed", cfg_pre, 2, 77), tap_spec("blocks.0.hook_resid_pre", cfg_pre, 2, 77)
    assert (full.slot, full.layer) == (pre0.slot, pre0.layer) == (S["FULL_EMBED"], 0)      # one buffer, as in the reference
    with pytest.raises(KeyError):
        tap_spec("hook_ln_pre", cfg, 2, 77)
