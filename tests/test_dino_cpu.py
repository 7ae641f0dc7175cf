"""The DINO family without a GPU: checkpoint conversion, registry entries, the pooled final stages on the PyTorch path and what
``NativeViT.supported`` says about long sequences and pooled heads.

Fixtures (tests/golden/gen_golden_dino.py, which executes the reference on the CPU):
* ``weight_conversion_dino_tiny.npz``  a seeded synthetic HuggingFace ``ViTModel`` checkpoint and what the reference's
  ``convert_dino_weights`` (models/weight_conversion.py:432-518) returned for it;
* ``model_registry_dino.json``         the four DINO entries of the reference's registry (models/model_config_registry.py:544-570);
* ``vit_tiny_pooled_heads.npz``        the reference's fp32 run of two tiny models, one with ``classification_type="gaap"`` and one named
  ``facebook/dino-vitb-tiny`` (``cat(cls, mean(patches))``, base_vit.py:195-208): output, hook_ln_final, hook_post_head_pre_normalize.

The arch tables and the synthetic checkpoint live here so that the generator, this file and tests/test_dino_gpu.py use the same ones.
"""
import json
import os
import re

import numpy as np
import torch

from vit_prisma_amd import HookedViT, HookedViTConfig, _native
from vit_prisma_amd.native_vit import NativeViT
from vit_prisma_amd.synth import ARCHS, synth_images, synth_vit_state

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# d_model 64, 2 layers, 2 heads, d_head 32, 17 tokens (32 px / 8); batch 3
POOLED_ARCHS = {
    "gaap": dict(ARCHS["tiny"], classification_type="gaap", model_name="synthetic-tiny-gaap"),
    "dino": dict(ARCHS["tiny"], classification_type="cls", model_name="facebook/dino-vitb-tiny", return_type="pre_logits",
                 layer_norm_pre=False, eps=1e-6),
}
POOLED_BATCH = 3
POOLED_KEYS = ("hook_ln_final", "hook_post_head_pre_normalize")


def rel_fro(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def pooled_model(tag: str, dtype=torch.float32, device="cpu", **overrides) -> HookedViT:
    arch = dict(POOLED_ARCHS[tag], **overrides)
    model = HookedViT(HookedViTConfig(**arch, dtype=dtype, device=device))
    if "image_size" not in overrides and "patch_size" not in overrides:        # (the seeded state has the tables' shapes)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in synth_vit_state(arch, seed=5).items() if k in model.state_dict()},
                              strict=True)
    return model.to(dtype).to(device).eval()


def dino_tiny_cfg() -> HookedViTConfig:
    return HookedViTConfig(**POOLED_ARCHS["dino"], device="cpu")


def synth_hf_vit_state(cfg, seed=0):
    """A state dict with HuggingFace ``ViTModel``'s key names and shapes (what ``ViTModel.from_pretrained("facebook/dino-...")`` holds)."""
    g = torch.Generator().manual_seed(seed)
    d, L, dm, p, C = cfg.d_model, cfg.n_layers, cfg.d_mlp, cfg.patch_size, cfg.n_channels
    T = (cfg.image_size // p) ** 2 + 1
    r = lambda *s, std=0.05: torch.randn(*s, generator=g) * std       # noqa: E731
    sd = {"embeddings.cls_token": r(1, 1, d, std=0.3), "embeddings.position_embeddings": r(1, T, d, std=0.3),
          "embeddings.patch_embeddings.projection.weight": r(d, C, p, p, std=(C * p * p) ** -0.5),
          "embeddings.patch_embeddings.projection.bias": r(d), "layernorm.weight": 1 + r(d), "layernorm.bias": r(d)}
    for l in range(L):
        k = f"encoder.layer.{l}"
        sd.update({k + ".layernorm_before.weight": 1 + r(d), k + ".layernorm_before.bias": r(d),
                   k + ".layernorm_after.weight": 1 + r(d), k + ".layernorm_after.bias": r(d),
                   k + ".attention.output.dense.weight": r(d, d, std=d ** -0.5), k + ".attention.output.dense.bias": r(d),
                   k + ".intermediate.dense.weight": r(dm, d, std=d ** -0.5), k + ".intermediate.dense.bias": r(dm),
                   k + ".output.dense.weight": r(d, dm, std=dm ** -0.5), k + ".output.dense.bias": r(d)})
        for nm in ("query", "key", "value"):
            sd.update({f"{k}.attention.attention.{nm}.weight": r(d, d, std=d ** -0.5), f"{k}.attention.attention.{nm}.bias": r(d)})
    return sd


def test_convert_dino_weights_equals_the_reference_converter_bitwise():
    from vit_prisma_amd.weights import convert_dino_weights
    G = np.load(os.path.join(GOLDEN, "weight_conversion_dino_tiny.npz"))
    cfg = dino_tiny_cfg()
    sd = synth_hf_vit_state(cfg, seed=4)
    for k, v in sd.items():                                          # the fixture's checkpoint is the one generated here
        assert np.array_equal(G["in_hf::" + k], v.numpy()), k
    got = convert_dino_weights(sd, cfg)
    want = {k[len("ref::"):]: G[k] for k in G.files if k.startswith("ref::")}
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        assert tuple(got[k].shape) == v.shape and np.array_equal(got[k].numpy(), v), k


def test_load_dino_weights_fills_a_model_and_the_forward_runs(tmp_path):
    from vit_prisma_amd.weights import convert_dino_weights, load_dino_weights
    cfg = dino_tiny_cfg()
    sd = synth_hf_vit_state(cfg, seed=4)
    path = str(tmp_path / "dino_tiny.pt")
    torch.save({"vit." + k: v for k, v in sd.items()}, path)          # (ViTForImageClassification checkpoints carry the prefix)
    model = load_dino_weights(HookedViT(cfg), path).eval()
    want = convert_dino_weights(sd, cfg)
    for k, v in want.items():
        assert torch.equal(model.state_dict()[k], v), k
    with torch.no_grad():
        out = model(torch.from_numpy(synth_images(POOLED_ARCHS["dino"], 2, 1)))
    assert out.shape == (2, cfg.d_model, 2) and bool(torch.isfinite(out).all())


def test_dino_registry_entries_equal_the_reference_registry():
    from vit_prisma_amd.model_loader import DINO_ARCH, list_available_models, load_config
    with open(os.path.join(GOLDEN, "model_registry_dino.json")) as f:
        reg = json.load(f)
    assert sorted(reg) == sorted(DINO_ARCH) == ["facebook/dino-vitb16", "facebook/dino-vitb8", "facebook/dino-vits16", "facebook/dino-vits8"]
    for name, fields in reg.items():
        assert name in list_available_models()
        cfg = load_config(name, device="cpu")
        assert cfg.model_name == name and cfg.d_head == cfg.d_model // cfg.n_heads      # (the reference's load_config :205-207)
        for k, v in fields.items():
            assert getattr(cfg, k) == v, (name, k, getattr(cfg, k), v)
    # the token counts the issue quotes: /16 -> 197, /8 -> 785
    for name, T in (("facebook/dino-vitb16", 197), ("facebook/dino-vits16", 197), ("facebook/dino-vitb8", 785), ("facebook/dino-vits8", 785)):
        cfg = load_config(name, device="cpu")
        assert (cfg.image_size // cfg.patch_size) ** 2 + 1 == T


def test_pooled_heads_on_the_pytorch_path_vs_reference_fixture():
    G = np.load(os.path.join(GOLDEN, "vit_tiny_pooled_heads.npz"))
    for tag, arch in POOLED_ARCHS.items():
        model = pooled_model(tag)
        x = torch.from_numpy(synth_images(arch, POOLED_BATCH, 1))
        with torch.no_grad():
            out, cache = model.run_with_cache(x)
        want = torch.from_numpy(G[f"{tag}::__out__"])
        assert out.shape == want.shape == ((POOLED_BATCH, 24) if tag == "gaap" else (POOLED_BATCH, 64, 2))
        assert rel_fro(out, want) < 1e-5, (tag, rel_fro(out, want))
        assert list(cache.keys()) == list(G[f"{tag}::__keys__"])
        for k in POOLED_KEYS:
            assert cache[k].shape == G[f"{tag}::{k}"].shape and rel_fro(cache[k], torch.from_numpy(G[f"{tag}::{k}"])) < 1e-5, (tag, k)


def _cfg(**kw):
    base = dict(ARCHS["tiny"], n_layers=1, patch_size=4)
    base.update(kw)
    return HookedViTConfig(**base, device="cpu")


def test_native_plan_accepts_dino_gaap_and_long_sequences():
    from vit_prisma_amd.model_loader import load_config
    for name in ("facebook/dino-vits8", "facebook/dino-vitb16", "facebook/dino-vitb8", "facebook/dino-vits16"):
        cfg = load_config(name, device="cpu")
        T = (cfg.image_size // cfg.patch_size) ** 2 + 1
        assert NativeViT.supported(cfg, T) is None, name
        assert NativeViT.supported(load_config(name, device="cpu", dtype=torch.bfloat16), T) is None, name
    assert NativeViT.supported(HookedViTConfig(**POOLED_ARCHS["gaap"], device="cpu"), 17) is None
    assert NativeViT.supported(HookedViTConfig(**POOLED_ARCHS["dino"], device="cpu"), 17) is None
    assert NativeViT.supported(_cfg(image_size=180), 2026) is None                      # 45 x 45 patches + cls: at the cap
    assert NativeViT.supported(_cfg(image_size=180, d_head=64, d_model=128), 2026) is None


def test_native_plan_refuses_beyond_the_cap_and_dino_vitb_with_a_head():
    why = NativeViT.supported(_cfg(image_size=184), 2117)                              # 46 x 46 + cls
    assert why is not None and "attention shape" in why
    why = NativeViT.supported(HookedViTConfig(**dict(POOLED_ARCHS["dino"], return_type="class_logits"), device="cpu"), 17)
    assert why is not None and "classification_type" in why and "head" in why
    assert NativeViT.supported(_cfg(classification_type="last_hidden"), 65) == "classification_type"


def test_the_token_cap_is_one_number():
    """include/pv_native.h's PV_ATTN_MAX_TOKENS, the Python binding's copy and what ``supported`` enforces are the same 2048; the
    library enforces it at plan creation with a message that states it."""
    import ctypes as C
    src = open(os.path.join(ROOT, "include", "pv_native.h")).read()
    cap = int(re.search(r"#define\s+PV_ATTN_MAX_TOKENS\s+(\d+)", src).group(1))
    assert cap == _native.ATTN_MAX_TOKENS == 2048
    assert NativeViT.supported(_cfg(use_cls_token=False, image_size=180), cap - 23) is None      # 2025 patches
    assert NativeViT.supported(_cfg(), cap + 1) == "attention shape"
    lib = _native.lib()
    mk = lambda img, pool, head: _native.VitDesc(n_layers=1, d_model=64, n_heads=2, d_head=32, d_mlp=128, n_channels=3, patch_size=4,  # noqa: E731
                                                  image_size=img, n_tokens=(img // 4) ** 2 + 1, n_classes=24, use_cls_token=1,
                                                  layer_norm_pre=1, has_head=head, normalize_output=1, activation=0, dtype=0, eps=1e-5,
                                                  attn_scale=32 ** 0.5, pooling=pool)
    plan = C.c_void_p()
    for pool, head in ((0, 1), (1, 1), (1, 0), (2, 0)):
        desc = mk(180, pool, head)
        assert lib.pv_vit_plan_create(C.byref(desc), C.byref(plan)) == 0, (pool, head, _native.last_error())
        assert lib.pv_vit_workspace_bytes(plan, 2) > 2 * 2026 * 64 * 4
        lib.pv_vit_plan_destroy(plan)
    desc = mk(184, 0, 1)
    assert lib.pv_vit_plan_create(C.byref(desc), C.byref(plan)) == 1 and str(cap) in _native.last_error()
    desc = mk(32, 2, 1)                                                  # cat(cls, mean(patches)) with a head
    assert lib.pv_vit_plan_create(C.byref(desc), C.byref(plan)) == 1 and "PV_POOL_CLS_MEAN" in _native.last_error()
    desc = mk(32, 3, 0)
    assert lib.pv_vit_plan_create(C.byref(desc), C.byref(plan)) == 1 and "pooling" in _native.last_error()
