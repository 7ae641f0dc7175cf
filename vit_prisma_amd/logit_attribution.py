"""Direct logit attribution by attention head on an all-hooks cache.

    attr, labels = head_logit_attribution(cache, answers, layer=None, pos=None)      # [B, T, layer * H, O] fp32, "L{l}H{h}"

What ``einsum(cache.stack_head_results(layer, apply_ln=True), answers)`` computes with the reference's helpers: every head's
``z[..., h, :] @ W_O[h]`` of the layers below ``layer``, centred, divided by the cached ``hook_scale`` of the LayerNorm those
heads feed (``blocks.{layer}.ln1``, or ``ln_final`` for ``None`` / ``-1`` / ``n_layers``) and multiplied with the answer
directions.  ``answers`` is ``[O, d_model]`` when every image shares the directions and ``[B, O, d_model]`` when each image has
its own (the unembedding row of its label, a logit difference).  ``pos`` selects one token of every image (``pos=0``: the CLS
row); the result then has one token.

On a bf16 model whose cache lives on the GPU this runs in ``pv_head_attribution`` (csrc/attribution.hip): the
centred answers are folded through ``W_O`` once and the ``hook_z`` taps are read once where they lie -- no ``[..., d_model]``
intermediate, every sum in fp32, the answers kept in fp32.  More than 16 answers run in chunks of 16.  Everything else -- fp32
models, CPU caches, caches without a batch dimension -- runs the reference's composition one layer at a time.  Which of the two
ran is in ``last_run_native`` / ``native_fallback_reason``; ``use_native(True)`` turns a fallback into an error.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Union

import torch

from . import _native

MAX_ANSWERS = 16                 # PV_ATTR_MAX_ANSWERS
MAX_LAYERS = 64                  # PV_ATTR_MAX_LAYERS

last_run_native: bool = False
native_fallback_reason: Optional[str] = None
_native_mode = "auto"            # "auto" | "off" | "force"


def use_native(mode: Union[bool, str, None]) -> None:
    """True/"force": raise unless the HIP path can run; False/"off": always PyTorch; None/"auto": the HIP path where it applies."""
    global _native_mode
    mode = {True: "force", False: "off", None: "auto"}.get(mode, mode)
    assert mode in ("auto", "off", "force")
    _native_mode = mode


def _resolve_layer(cache, layer: Optional[int]) -> int:
    n_layers = cache.model.cfg.n_layers
    if layer is None or layer == -1:
        return n_layers
    if not 0 <= layer <= n_layers:
        raise IndexError(f"layer {layer} is outside 0 .. {n_layers}")
    return int(layer)


def _scale_key(cache, layer: int) -> str:
    return "ln_final.hook_scale" if layer == cache.model.cfg.n_layers else f"blocks.{layer}.ln1.hook_scale"


def _native_reason(cache, answers: torch.Tensor, layer: int, pos: Optional[int]) -> Optional[str]:
    """None when ``pv_head_attribution`` serves this call, else why it does not."""
    cfg = cache.model.cfg
    if not cache.has_batch_dim:
        return "the cache has no batch dimension"
    if cfg.normalization_type != "LN":
        return f"normalization_type is {cfg.normalization_type!r}, not 'LN'"
    if cfg.dtype != torch.bfloat16:
        return f"the model is {cfg.dtype}, the HIP attribution serves bf16"
    if cfg.d_model % 8 != 0:
        return "d_model is not a multiple of 8"
    dh = cfg.d_head
    if not (dh in (32, 64) or (64 < dh <= 128 and dh % 8 == 0)):
        return f"d_head {dh} is not 32, 64 or a multiple of 8 in (64, 128]"
    if not 1 <= layer <= MAX_LAYERS:
        return f"{layer} layers below `layer`: the HIP attribution serves 1 .. {MAX_LAYERS}"
    keys = [f"blocks.{l}.attn.hook_z" for l in range(layer)]
    scale_key = _scale_key(cache, layer)
    missing = [k for k in keys + [scale_key] if k not in cache.cache_dict]
    if missing:
        return f"the cache lacks {missing[0]}"
    first = cache.cache_dict[keys[0]]
    if not first.is_cuda:
        return "the cache is not on a GPU"
    for k in keys:
        t = cache.cache_dict[k]
        if (t.dtype != torch.bfloat16 or t.dim() != 4 or t.shape != first.shape or t.device != first.device
                or not t.is_contiguous() or tuple(t.shape[2:]) != (cfg.n_heads, dh) or t.data_ptr() % 16):
            return f"{k} is not a contiguous, 16-byte aligned [B, T, H, d_head] bf16 tensor on the cache's device"
    if first.numel() * 2 >= 1 << 32:
        return "a hook_z tap holds 4 GiB or more"
    scale = cache.cache_dict[scale_key]
    if (scale.dtype != torch.float32 or scale.shape != (*first.shape[:2], 1) or scale.device != first.device
            or not scale.is_contiguous()):
        return f"{scale_key} is not a contiguous fp32 [B, T, 1] tensor on the cache's device"
    for l in range(layer):
        w = cache.model.blocks[l].attn.W_O
        if (w.dtype != torch.bfloat16 or tuple(w.shape) != (cfg.n_heads, dh, cfg.d_model) or w.device != first.device
                or not w.is_contiguous() or w.data_ptr() % 16):
            return f"blocks.{l}.attn.W_O is not a contiguous, 16-byte aligned bf16 [H, d_head, d_model] tensor on the cache's device"
    if not answers.is_floating_point() or answers.shape[-2] == 0:
        return "answers is not a floating-point tensor with at least one row"
    if answers.device != first.device:
        return "answers is not on the cache's device"
    if pos is not None and not 0 <= pos < first.shape[1]:
        return f"pos {pos} is not a token of the cache"
    if torch.is_grad_enabled() and (answers.requires_grad or any(cache.cache_dict[k].requires_grad for k in keys)
                                    or any(cache.model.blocks[l].attn.W_O.requires_grad for l in range(layer))):
        return "autograd is recording"
    if not _native.available():
        return "libpvnative.so is not built"
    return None


def _dispatch(cache, answers: torch.Tensor, layer: int, pos: Optional[int]) -> bool:
    global last_run_native, native_fallback_reason
    if _native_mode == "off":
        last_run_native, native_fallback_reason = False, "native_mode == 'off'"
        return False
    reason = _native_reason(cache, answers, layer, pos)
    if reason is not None and _native_mode == "force":
        raise _native.NativeError(f"native head attribution impossible: {reason}")
    last_run_native, native_fallback_reason = reason is None, reason
    return reason is None


def _run_native(cache, answers: torch.Tensor, layer: int, pos: Optional[int]) -> torch.Tensor:
    """``pv_head_attribution`` on the whole batch, one call per 16 answers."""
    cfg = cache.model.cfg
    taps = [cache.cache_dict[f"blocks.{l}.attn.hook_z"] for l in range(layer)]
    weights = [cache.model.blocks[l].attn.W_O.detach() for l in range(layer)]
    scale = cache.cache_dict[_scale_key(cache, layer)]
    B, T, H, dh = taps[0].shape
    per_image = answers.dim() == 3
    O = answers.shape[-2]
    t_out = T if pos is None else 1
    dev = taps[0].device
    answers = answers.detach().to(torch.float32)
    lib = _native.lib()
    z_ptrs = (C.c_void_p * layer)(*[t.data_ptr() for t in taps])
    w_ptrs = (C.c_void_p * layer)(*[w.data_ptr() for w in weights])
    chunks: List[torch.Tensor] = []
    with torch.cuda.device(dev):
        for o0 in range(0, O, MAX_ANSWERS):
            a = answers[..., o0:o0 + MAX_ANSWERS, :].contiguous()
            if a.data_ptr() % 16:
                a = a.clone()                                              # (a view at an odd offset: the kernels load 16 bytes)
            n = a.shape[-2]
            ws_bytes = lib.pv_head_attribution_workspace_bytes(layer, H, dh, B * n if per_image else n)
            ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
            out = torch.empty((B, t_out, layer * H, n), dtype=torch.float32, device=dev)
            rc = lib.pv_head_attribution(_native.PV_DTYPE_BF16, z_ptrs, w_ptrs, layer, B, T, -1 if pos is None else int(pos), H, dh,
                                         cfg.d_model, scale.data_ptr(), a.data_ptr(), n, 1 if per_image else 0, out.data_ptr(),
                                         ws.data_ptr(), ws_bytes, torch.cuda.current_stream(dev).cuda_stream)
            _native.check(rc, "pv_head_attribution")
            # (the stream orders the kernels before any later use or reuse of `ws` / `a` memory: the caching allocator hands a
            # freed block to work on the same stream only)
            chunks.append(out)
    return chunks[0] if len(chunks) == 1 else torch.cat(chunks, dim=-1)


def _times_answers(stack: torch.Tensor, answers: torch.Tensor, per_image: bool) -> torch.Tensor:
    """[C, ..., d_model] x answers -> [C, ..., O], the operands brought to their common dtype first (torch.einsum takes no mix)"""
    dtype = torch.promote_types(stack.dtype, answers.dtype)
    return torch.einsum("cbtd,bod->cbto" if per_image else "c...d,od->c...o", stack.to(dtype), answers.to(dtype))


def _run_torch(cache, answers: torch.Tensor, layer: int, pos: Optional[int]) -> torch.Tensor:
    """The reference's composition -- compute_head_results, stack_head_results(apply_ln=True), the product with the answers -- one
    layer at a time, so that no more than one layer's [..., H, d_model] exists at once."""
    cfg = cache.model.cfg
    scale = None
    if cfg.normalization_type in ("LN", "LNPre"):
        scale = cache[_scale_key(cache, layer)]
        if pos is not None:
            scale = scale[..., pos:pos + 1, :]
    per_image = answers.dim() == 3
    parts = []
    for l in range(layer):
        key = f"blocks.{l}.attn.hook_result"
        if key in cache.cache_dict:
            res = cache.cache_dict[key]
        else:
            res = torch.einsum("...he,hed->...hd", cache[("z", l, "attn")], cache.model.blocks[l].attn.W_O)
        if pos is not None:
            res = res[..., pos:pos + 1, :, :]
        res = res.movedim(-2, 0)                                           # [H, ..., pos, d_model]
        if scale is not None:
            res = (res - res.mean(dim=-1, keepdim=True)) / scale
        parts.append(res if pos is not None else _times_answers(res, answers, per_image))
    if parts and pos is not None:
        # one token per image: the L * H rows per image are few, so they are multiplied in one product, not in L small ones
        return _times_answers(torch.cat(parts, dim=0), answers, per_image).movedim(0, -2)
    if not parts:
        ref = cache[("resid_post", layer - 1)] if layer > 0 else cache[("resid_pre", 0)]
        lead = ref.shape[:-2] + ((ref.shape[-2] if pos is None else 1),)
        dtype = torch.promote_types(ref.dtype if scale is None else torch.promote_types(ref.dtype, scale.dtype), answers.dtype)
        return torch.zeros((*lead, 0, answers.shape[-2]), dtype=dtype, device=ref.device)
    return torch.cat(parts, dim=0).movedim(0, -2)


def head_logit_attribution(cache, answers: torch.Tensor, layer: Optional[int] = None, pos: Optional[int] = None,
                           return_labels: bool = True):
    """``(attr [B, T, layer * H, O], labels)``: what every attention head of the layers below ``layer`` writes along each answer
    direction after the LayerNorm scaling of the layer it feeds; ``[B, 1, layer * H, O]`` with ``pos``.  ``answers``: ``[O,
    d_model]`` shared, or ``[B, O, d_model]`` per image.  Labels ``"L{l}H{h}"`` as in ``stack_head_results``."""
    cfg = cache.model.cfg
    layer = _resolve_layer(cache, layer)
    if answers.dim() not in (2, 3) or answers.shape[-1] != cfg.d_model:
        raise ValueError(f"answers must be [O, d_model] or [B, O, d_model] with d_model = {cfg.d_model}, not {tuple(answers.shape)}")
    if answers.dim() == 3:
        if not cache.has_batch_dim:
            raise ValueError("answers per image need a cache with a batch dimension")
        n_images = cache[("z", 0, "attn")].shape[0]
        if answers.shape[0] != n_images:
            raise ValueError(f"answers hold {answers.shape[0]} images, the cache {n_images}")
    if pos is not None:
        pos = int(pos)
    labels = [f"L{l}H{h}" for l in range(layer) for h in range(cfg.n_heads)]
    if _dispatch(cache, answers, layer, pos):
        attr = _run_native(cache, answers, layer, pos).to(torch.promote_types(torch.float32, answers.dtype))
    else:
        attr = _run_torch(cache, answers, layer, pos)
    return (attr, labels) if return_labels else attr
