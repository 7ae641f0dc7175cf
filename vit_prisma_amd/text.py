"""HookedTextTransformer -- CLIP's text tower with a HookPoint on every intermediate activation.

Drop-in for the reference's class (/root/reference/src/vit_prisma/models/base_text_transformer.py:24-223): module / parameter /
HookPoint names, signatures and hook semantics identical, state dicts interchange.  Built from vit.py's layers; the causal mask is
the reference's additive buffer (-inf above the diagonal, :188-194) handed to every block.

Pure caching calls (``run_with_cache`` without user hooks) and the plain ``model(tokens)`` call on a GPU, outside autograd, with
``tokens.shape[1] == cfg.context_length`` run on the native HIP plan (``native_vit.NativeText`` -> pv_text_forward): token embedding,
the ViT's block sequence under ``attn_causal_kernel``, ln_final, the row at the EOT token, head.  Everything else takes the PyTorch
path below, with the reason in ``native_fallback_reason``.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple, Union

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _native
from .activation_cache import ActivationCache
from .configs import HookedTextTransformerConfig
from .hook_points import HookPoint
from .hooked_root_module import HookedRootModule, names_filter_to_fn
from .vit import MLP, Attention, Head, LayerNorm, PosEmbedding, TransformerBlock, _make_norm

HOOKS_REASON = ("forward hooks on a text model run on the PyTorch path: splitting the plan at hook points is split_plan's job and "
                "is not wired to the text plan")


class HookedTextTransformer(HookedRootModule):
    """Base text model."""

    def __init__(self, cfg: Union[HookedTextTransformerConfig, Dict], no_causal_mask: bool = False, proj_type: str = "linear",
                 cls_token: bool = False):
        super().__init__()
        if isinstance(cfg, dict):
            cfg = HookedTextTransformerConfig(**cfg)
        elif isinstance(cfg, str):
            raise ValueError("Please pass in a config dictionary or HookedTextTransformerConfig object.")
        if cls_token:
            # the reference's own forward tests `if self.cls_emb:` on a multi-element Parameter (base_text_transformer.py:129),
            # which raises: there is no behaviour to reproduce
            raise NotImplementedError("cls_token=True: the reference's forward raises on it (truth value of a multi-element Parameter)")
        self.cfg = cfg
        self.num_pos = self.context_length = cfg.context_length
        self.token_embed = nn.Embedding(cfg.vocab_size, cfg.d_model)
        self.hook_embed = HookPoint()
        self.pad_id = 0
        self.pos_embed = nn.Parameter(torch.empty(self.num_pos, cfg.d_model))
        self.hook_pos_embed = HookPoint()
        self.cls_emb = None
        self.hook_full_embed = HookPoint()
        if cfg.normalization_type != "LN":
            raise ValueError(f"Invalid normalization type: {cfg.normalization_type}")
        self.ln_pre = LayerNorm(cfg)              # (exists, never runs: base_text_transformer.py:65-71, 119-160)
        self.hook_ln_pre = HookPoint()
        self.blocks = nn.ModuleList([TransformerBlock(cfg, i) for i in range(cfg.n_layers)])
        self.ln_final = _make_norm(cfg)
        self.hook_ln_final = HookPoint()
        if no_causal_mask:
            self.attn_mask = None
        else:
            self.register_buffer("attn_mask", self.build_causal_mask(), persistent=False)
        self.head = Head(cfg)
        self.hook_post_head_pre_normalize = HookPoint()
        self.init_weights()
        self.setup()
        # native (HIP) execution state
        self._module_signature = [(m, tuple(m._modules.items())) for m in self.modules() if m._modules]
        self._plain_modules = [m for m in self.modules() if not isinstance(m, HookPoint)]
        self.native_mode = "auto"            # "auto" | "off" | "force"
        self._native = None
        self.last_run_native = False
        self.native_fallback_reason: Optional[str] = None

    # ------------------------------------------------------------------------------ PyTorch path
    def forward(self, input: torch.Tensor, attn_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        if not getattr(self, "_in_cache_fallback", False):
            reason = self._native_reason((input,), {})
            if reason is None:
                out, _ = self._run_native(input, names_filter=[])
                self.last_run_native, self.native_fallback_reason = True, None
                return out
            if self.native_mode == "force":
                raise _native.NativeError(f"native forward impossible: {reason}")
            self.last_run_native, self.native_fallback_reason = False, reason
        seq_len = input.shape[1]
        token_embed = self.hook_embed(self.token_embed(input))
        attn_mask = self.attn_mask                           # (the argument is ignored, as in the reference: :127)
        pos_embed = self.hook_pos_embed(self.pos_embed[:seq_len])
        x = token_embed + pos_embed
        self.hook_full_embed(x)                              # observe-only (return value unused)
        for block in self.blocks:
            x = block(x, attn_mask=attn_mask)
        x = self.ln_final(x)
        self.hook_ln_final(x)                                # observe-only
        x = x[torch.arange(x.shape[0]), input.argmax(dim=-1)]
        x = x if self.cfg.return_type == "pre_logits" else self.head(x)
        self.hook_post_head_pre_normalize(x)                 # observe-only
        if self.cfg.normalize_output:
            x = F.normalize(x, dim=-1)
        return x

    def build_causal_mask(self) -> torch.Tensor:
        # additive mask: -inf above the diagonal, 0 elsewhere (base_text_transformer.py:188-194)
        mask = torch.empty(self.num_pos, self.num_pos)
        mask.fill_(float("-inf"))
        mask.triu_(1)
        return mask

    def init_weights(self) -> None:
        cfg = self.cfg
        nn.init.normal_(self.token_embed.weight, std=0.02)
        nn.init.normal_(self.pos_embed, std=0.01)
        if cfg.weight_type != "he":
            return
        for m in self.modules():
            if isinstance(m, PosEmbedding):
                nn.init.normal_(m.W_pos, std=cfg.pos_std)
            elif isinstance(m, Attention):
                for w in (m.W_Q, m.W_K, m.W_V, m.W_O):
                    nn.init.xavier_uniform_(w)
            elif isinstance(m, MLP):
                nn.init.kaiming_normal_(m.W_in, nonlinearity="relu")
                nn.init.kaiming_normal_(m.W_out, nonlinearity="relu")
                nn.init.zeros_(m.b_out)
                nn.init.zeros_(m.b_in)
            elif isinstance(m, Head):
                nn.init.kaiming_normal_(m.W_H, nonlinearity="relu")
                nn.init.zeros_(m.b_H)
            elif isinstance(m, (nn.Linear, nn.Conv2d)):
                nn.init.kaiming_normal_(m.weight, nonlinearity="relu")
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    # ------------------------------------------------------------------------------ native path
    def use_native(self, mode: Union[bool, str, None]) -> "HookedTextTransformer":
        """True/"force": raise unless the HIP path can run; False/"off": always PyTorch hooks; None/"auto": HIP path whenever the
        call is a pure caching call (or a plain forward) on a GPU."""
        self.native_mode = {True: "force", False: "off", None: "auto"}.get(mode, mode)
        assert self.native_mode in ("auto", "off", "force")
        return self

    def invalidate_native_weights(self) -> None:
        """Force a repack of the weight shadow on the next native call (after edits through ``param.data``)."""
        if self._native is not None:
            self._native._weights_key = None

    def freeze_native_weights(self, frozen: bool = True) -> None:
        """Promise that parameters do not change (skips the per-call change detection)."""
        self._native_frozen = frozen
        if self._native is not None:
            self._native.freeze_weights(frozen)

    def _tree_matches(self) -> bool:
        return all(tuple(m._modules.items()) == kids for m, kids in self._module_signature)

    def _native_reason(self, model_args, kwargs) -> Optional[str]:
        """None when the call can run on the native plan, else why not (each cause its own text)."""
        if self.native_mode == "off":
            return "native_mode == 'off'"
        if len(model_args) != 1 or not isinstance(model_args[0], torch.Tensor):
            return "positional arguments"
        x = model_args[0]
        extra = set(kwargs) - {"names_filter", "device", "incl_bwd", "reset_hooks_end", "clear_contexts", "fwd_hooks", "bwd_hooks"}
        if extra:
            return f"unsupported kwargs {sorted(extra)}"
        if kwargs.get("incl_bwd", False) or kwargs.get("bwd_hooks"):
            return "backward hooks requested"
        if kwargs.get("fwd_hooks"):
            return HOOKS_REASON
        if not self._tree_matches():
            return "the module tree was modified after construction (spliced / replaced sub-modules)"
        if not x.is_cuda:
            return "input is not on a GPU"
        if self.pos_embed.device != x.device:
            return "model and input on different devices"
        if x.is_floating_point() or x.is_complex() or x.dtype == torch.bool:
            return f"token ids must be integers, got {x.dtype}"
        if x.ndim != 2 or x.shape[1] != self.cfg.context_length:
            return f"tokens.shape[1] != context_length ({tuple(x.shape)} against {self.cfg.context_length})"
        cfg = self.cfg
        if cfg.use_attn_result or cfg.use_split_qkv_input or cfg.use_hook_mlp_in or cfg.use_attn_in:
            return "flag-gated hook points (use_attn_result / use_split_qkv_input / use_hook_mlp_in / use_attn_in) are enabled"
        if self.training and (cfg.attn_dropout_rate or cfg.mlp_dropout_rate):
            return "dropout active in training mode"
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return "autograd is recording (use torch.no_grad() / requires_grad_(False))"
        for hp in self.hook_dict.values():
            if hp._forward_hooks or hp._backward_hooks:
                return HOOKS_REASON
        for mod in self._plain_modules:
            if mod._forward_hooks or mod._forward_pre_hooks:
                return "nn.Module hooks registered"
        from .native_vit import NativeText
        why = NativeText.supported(cfg)
        if why:
            return f"unsupported configuration: {why}"
        try:
            self._get_native(x.device)
        except _native.NativeError as e:                     # (the plan's own rule, in its own words)
            return f"unsupported shape: {e}"
        return None

    def _get_native(self, device: torch.device):
        from .native_vit import NativeText
        nv = self._native
        if nv is None or nv.device != device or nv.cfg.dtype != self.cfg.dtype:
            nv = NativeText(self.cfg, device, causal=self.attn_mask is not None)
            nv.freeze_weights(getattr(self, "_native_frozen", False))
            self._native = nv
        return nv

    def _run_native(self, tokens: torch.Tensor, names_filter=None, device=None, remove_batch_dim: bool = False,
                    **_ignored) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
        from .tap_plan import hook_order
        keep = names_filter_to_fn(names_filter)
        wanted = [n for n in hook_order(self.cfg, self.cfg.n_layers, True) if keep(n)]
        return self._get_native(tokens.device).forward(self, tokens, wanted, self.cfg.n_layers, True, cache_device=device,
                                                       remove_batch_dim=remove_batch_dim)

    def run_with_cache(self, *model_args, return_cache_object: bool = True, remove_batch_dim: bool = False,
                       **kwargs) -> Tuple[torch.Tensor, Union[ActivationCache, Dict[str, torch.Tensor]]]:
        """Same contract as base_text_transformer.py:162-186 + hooked_root_module.py:255-287; pure caching calls on a GPU run on
        the native plan, every requested activation written once by the kernel that produces it."""
        reason = self._native_reason(model_args, kwargs)
        if reason is None:
            out, cache_dict = self._run_native(model_args[0], remove_batch_dim=remove_batch_dim, **kwargs)
            self.last_run_native, self.native_fallback_reason = True, None
        else:
            if self.native_mode == "force":
                raise _native.NativeError(f"native run_with_cache impossible: {reason}")
            self.last_run_native, self.native_fallback_reason = False, reason
            self._in_cache_fallback = True
            try:
                out, cache_dict = super().run_with_cache(*model_args, remove_batch_dim=remove_batch_dim, **kwargs)
            finally:
                self._in_cache_fallback = False
        if return_cache_object:
            return out, ActivationCache(cache_dict, self, has_batch_dim=not remove_batch_dim)
        return out, cache_dict
