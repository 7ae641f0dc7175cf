"""vit_prisma_amd -- MI355X-native run_with_cache + SAE training path behind ViT-Prisma's API.

    from vit_prisma_amd import HookedViT, HookedViTConfig, ActivationCache, HookPoint

The arithmetic of the hot path lives in libpvnative.so (hand-written HIP for gfx950, C ABI in
include/pv_native.h); this package is the host-side mirror of the reference's Python interface.
"""
from .activation_cache import ActivationCache
from .configs import HookedTextTransformerConfig, HookedViTConfig
from .hook_points import HookPoint, LensHandle
from .hooked_root_module import HookedRootModule
from .compat import install_as
from .vit import (Attention, Head, HookedViT, LayerNorm, LayerNormPre, MLP, PatchEmbedding, PosEmbedding,
                  TransformerBlock)
from .sae_vit import HookedSAEViT
from .text import HookedTextTransformer
from . import logit_lens
from . import logit_attribution
from .logit_attribution import head_logit_attribution, neuron_logit_attribution, top_neuron_logit_attribution

__all__ = [
    "logit_lens", "logit_attribution", "head_logit_attribution", "neuron_logit_attribution", "top_neuron_logit_attribution",
    "ActivationCache", "HookedViTConfig", "HookPoint", "LensHandle", "HookedRootModule", "HookedViT", "HookedSAEViT",
    "HookedTextTransformer", "HookedTextTransformerConfig",
    "Attention", "Head", "LayerNorm", "LayerNormPre", "MLP", "PatchEmbedding", "PosEmbedding",
    "TransformerBlock", "install_as",
]
