"""``load_hooked_model`` for the two target architectures, OFFLINE (drop-in for the notebook entry point
/root/reference/src/vit_prisma/models/model_loader.py:278-368; aliased as ``vit_prisma.models.model_loader`` by ``install_as``).

The reference resolves ``model_name`` to a config and to weights by downloading from HuggingFace (model_loader.py:397-407, 775-784);
there is no network here.  This loader therefore takes the config from the architecture tables of ``synth.ARCHS`` plus the
per-name overrides of the reference registry (``NAME_OVERRIDES``) -- what ``load_config`` would have produced for these names, SURVEY.md 8a -- and the weights from a LOCAL open_clip / HuggingFace CLIP checkpoint, or for the DINO names (``DINO_ARCH``) a HuggingFace ``ViTModel`` one; the wide-head open_clip towers H/14, g/14 and bigG/14 are ``WIDE_ARCH``
(``local_path=...``: a ``.safetensors`` / ``.pt`` / ``.bin`` file, converted by ``weights.py`` exactly as the reference's converters do) --
or none (``pretrained=False``: the reference's initialisation).  Everything else about the signature is the reference's; the options
that rewrite weights (``fold_ln``, ``center_writing_weights``, ``refactor_factored_attn_matrices``) are not implemented and raise
when set; ``fold_value_biases`` (on by default, as in the reference: b_O absorbs the value biases, model_loader.py:286, 352-358 ->
base_vit.py:498-532) IS applied to loaded weights -- ``attn.hook_v`` / ``hook_z`` of a loaded model are those of the folded weights.
"""
from __future__ import annotations

import logging
from typing import Any, Optional, Type

import torch

from .configs import HookedTextTransformerConfig, HookedViTConfig
from .synth import ARCHS
from .vit import HookedViT
from .weights import load_clip_vision_weights, load_dino_weights

# reference model names (model_loader.py:97-123) -> architecture table
MODEL_ARCH = {
    "open-clip:laion/CLIP-ViT-B-32-DataComp.XL-s13B-b90K": "clip-vit-b32",
    "open-clip:laion/CLIP-ViT-B-32-DataComp.M-s128M-b4K": "clip-vit-b32",
    "open-clip:laion/CLIP-ViT-B-32-DataComp.S-s13M-b4K": "clip-vit-b32",
    "open-clip:laion/CLIP-ViT-B-32-laion2B-s34B-b79K": "clip-vit-b32",
    "openai/clip-vit-base-patch32": "clip-vit-b32",
    "openai/clip-vit-large-patch14-336": "clip-vit-l14-336",
}
# per-name overrides the reference registry applies on top of the architecture (models/model_config_registry.py:83-92, applied by
# its load_config :201-203): the HuggingFace OpenAI B/32 entry runs with eps = 1e-6 and WITHOUT the L2-normalised output, unlike the
# open_clip B/32 entries (BASE_OPEN_CLIP_CONFIGS["ViT-B"], :43-49).  Pinned by tests/golden/model_registry.json (values read out of
# the reference's registry by tests/golden/gen_golden_model_registry.py).
NAME_OVERRIDES = {
    "openai/clip-vit-base-patch32": {"eps": 1e-6, "normalize_output": False},
}
# the DINO family (registry DINO_CONFIGS, :544-570): HuggingFace ViTModel checkpoints, converted by weights.convert_dino_weights.  The
# registry's fields for these names are pinned by tests/golden/model_registry_dino.json (tests/golden/gen_golden_dino.py).  The vitb
# names return cat(cls, mean(patches)) -- [B, 768, 2] (base_vit.py:199-206).
DINO_ARCH = {
    "facebook/dino-vitb16": "dino-vitb16",
    "facebook/dino-vitb8": "dino-vitb8",
    "facebook/dino-vits16": "dino-vits16",
    "facebook/dino-vits8": "dino-vits8",
}
# the wide-head open_clip towers (registry :253-258, :326-328 over BASE_OPEN_CLIP_CONFIGS :58-78): heads of 80, 88 and 104, open_clip
# checkpoints like the B/32 names.  Pinned by tests/golden/model_registry_wide.json (tests/golden/gen_golden_vit_wide.py).
WIDE_ARCH = {
    "open-clip:laion/CLIP-ViT-H-14-laion2B-s32B-b79K": "clip-vit-h14",
    "open-clip:laion/CLIP-ViT-g-14-laion2B-s34B-b88K": "clip-vit-g14",
    "open-clip:laion/CLIP-ViT-bigG-14-laion2B-39B-b160k": "clip-vit-bigg14",
}
# the text towers of the reference's registry (OPEN_CLIP_TEXT_CONFIGS, models/model_config_registry.py:605-674): every one d_head 64
# at context 77.  The fields are the registry's, pinned by tests/golden/model_registry_text.json (tests/golden/gen_golden_text.py);
# served by load_text_config / list_available_text_models, NOT by load_config / list_available_models (whose values stay as they are).
BASE_TEXT_CONFIG = dict(d_model=768, n_heads=12, n_layers=12, d_mlp=3072, d_head=64, vocab_size=49408, context_length=77, eps=1e-5,
                        normalization_type="LN", layer_norm_pre=True)
_XLM_LARGE = dict(d_model=1024, n_heads=16, n_layers=24, d_mlp=4096, vocab_size=250002)
TEXT_CONFIGS = {
    "open-clip:laion/CLIP-ViT-B-32-DataComp.XL-s13B-b90K": {},
    "open-clip:laion/CLIP-ViT-L-14-DataComp.XL-s13B-b90K": {},
    "open-clip:laion/CLIP-ViT-B-32-xlm-roberta-base-laion5B-s13B-b90k": {"vocab_size": 250002},
    "open-clip:laion/CLIP-ViT-B-32-roberta-base-laion2B-s12B-b32k": {"vocab_size": 50265},
    "open-clip:laion/CLIP-ViT-H-14-frozen-xlm-roberta-large-laion5B-s13B-b90k": _XLM_LARGE,
    "open-clip:laion/CLIP-ViT-B-16-CommonPool.L-s1B-b8K": {},
    "open-clip:laion/CLIP-ViT-B-16-CommonPool.L.basic-s1B-b8K": {},
    "open-clip:laion/CLIP-ViT-B-16-CommonPool.L.clip-s1B-b8K": {},
    "open-clip:laion/CLIP-ViT-B-16-CommonPool.L.laion-s1B-b8K": {},
    "open-clip:laion/CLIP-ViT-B-32-CommonPool.M-s128M-b4K": {},
    "open-clip:laion/CLIP-ViT-B-32-CommonPool.S-s13M-b4K": {},
    "open-clip:laion/CLIP-ViT-L-14-CommonPool.XL-s13B-b90K": {},
    "open-clip:laion/CoCa-ViT-B-32-laion2B-s13B-b90k": {},
    "open-clip:laion/CoCa-ViT-L-14-laion2B-s13B-b90k": {},
}
DTYPE_FROM_STRING = {"float32": torch.float32, "fp32": torch.float32, "float16": torch.float16, "fp16": torch.float16,
                     "bfloat16": torch.bfloat16, "bf16": torch.bfloat16}


def list_available_models():
    return sorted({**MODEL_ARCH, **DINO_ARCH, **WIDE_ARCH})


def load_config(model_name: str, dtype: torch.dtype = torch.float32, device: str = "cuda", **overrides) -> HookedViTConfig:
    if model_name not in MODEL_ARCH and model_name not in DINO_ARCH and model_name not in WIDE_ARCH:
        raise ValueError(f"{model_name!r}: offline build knows {list_available_models()} (no network: configs cannot be downloaded)")
    kw = dict(ARCHS[MODEL_ARCH.get(model_name) or DINO_ARCH.get(model_name) or WIDE_ARCH[model_name]])
    kw["model_name"] = model_name
    kw.update(NAME_OVERRIDES.get(model_name, {}))
    kw.update(overrides)
    return HookedViTConfig(**kw, dtype=dtype, device=device)


def list_available_text_models():
    return sorted(TEXT_CONFIGS)


def load_text_config(model_name: str, dtype: torch.dtype = torch.float32, device: str = "cuda", **overrides) -> HookedTextTransformerConfig:
    """The registry's text config of ``model_name`` (its fields over the dataclass defaults, as the reference's load_config applies
    them); everything the registry leaves to the checkpoint (n_classes = the joint width, ...) comes in through ``overrides``."""
    if model_name not in TEXT_CONFIGS:
        raise ValueError(f"{model_name!r}: no text tower in the registry; known: {list_available_text_models()}")
    kw = {**BASE_TEXT_CONFIG, **TEXT_CONFIGS[model_name], "model_name": model_name}
    kw.update(overrides)
    return HookedTextTransformerConfig(**kw, dtype=dtype, device=device)


def load_hooked_model(model_name: str, model_class: Optional[Type] = None, model_type: Any = None, device: str = "cuda",
                      dtype: torch.dtype = torch.float32, pretrained: bool = True, fold_ln: bool = False,
                      center_writing_weights: bool = False, fold_value_biases: bool = True,
                      refactor_factored_attn_matrices: bool = False, move_to_device: bool = True, use_attn_result: bool = False,
                      allow_failing: bool = False, local_path: Optional[str] = None, **kwargs) -> HookedViT:
    assert not (kwargs.get("load_in_8bit", False) or kwargs.get("load_in_4bit", False)), "Quantization not supported"
    if isinstance(dtype, str):
        dtype = DTYPE_FROM_STRING[dtype]
    if "torch_dtype" in kwargs:
        dtype = kwargs.pop("torch_dtype")
    if fold_ln or center_writing_weights or refactor_factored_attn_matrices:
        raise NotImplementedError("fold_ln / center_writing_weights / refactor_factored_attn_matrices are not implemented in this build")
    if model_type is not None and str(getattr(model_type, "name", model_type)).upper() not in ("VISION", "MODELTYPE.VISION"):
        raise NotImplementedError("load_hooked_model builds the vision tower; the text tower is HookedTextTransformer(load_text_config(name, ...)) "
                                  "with weights from weights.convert_open_clip_text_weights")
    # cfg.dtype is set too: the reference's loader forgets it and its bf16 forward raises -- deliberate fix
    cfg = load_config(model_name, dtype=dtype, device=device)
    model = (model_class or HookedViT)(cfg)
    if pretrained:
        if local_path is None:
            raise FileNotFoundError(f"pretrained=True needs local_path=<checkpoint file> for {model_name!r}: this build cannot download "
                                    "weights (no network); pass pretrained=False for the reference's random initialisation")
        if model_name in DINO_ARCH:
            load_dino_weights(model, local_path, fold_value_biases=bool(fold_value_biases))
        else:
            load_clip_vision_weights(model, local_path, fold_value_biases=bool(fold_value_biases))
    model = model.to(dtype)
    if move_to_device:
        model = model.to(device)
    model.set_use_attn_result(use_attn_result)
    logging.info(f"Loaded {'pretrained ' if pretrained else ''}model {model_name} into HookedViT")
    return model
