"""Direct logit attribution by attention head and by MLP neuron on an all-hooks cache.

    attr, labels = head_logit_attribution(cache, answers, layer=None, pos=None)      # [B, T, layer * H, O] fp32, "L{l}H{h}"
    attr, labels = neuron_logit_attribution(cache, answers, layer=None, pos=None)    # [B, T, layer * d_mlp, O] fp32, "L{l}N{n}"
    top = top_neuron_logit_attribution(cache, answers, k, layer=None, pos=None, by="value")   # (values, layer, neuron) [B, T, O, k]

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

The neuron functions compute ``einsum(cache.stack_neuron_results(layer, apply_ln=True), answers)`` -- a stack of
``[layer * d_mlp, B, T, d_model]`` that nobody can hold at a useful size -- with the same answers, ``layer``, ``pos``, scale and
dispatch.  A neuron's result is one row of ``W_out`` times a number, so after the same fold (through ``mlp.W_out``) the value is
``post * G / scale`` per element: ``pv_neuron_attribution`` writes the dense tensor, ``pv_neuron_attribution_topk`` only the ``k``
largest per token and answer (csrc/attribution_neuron.hip).  Their PyTorch path runs the composition one layer at
a time in chunks of neurons and, for the top-k, orders the dense result.
"""
from __future__ import annotations

import collections
import ctypes as C
from typing import List, Optional, Union

import torch

from . import _native

MAX_ANSWERS = 16                 # PV_ATTR_MAX_ANSWERS
MAX_LAYERS = 64                  # PV_ATTR_MAX_LAYERS
MAX_TOPK = 256                   # PV_NATTR_MAX_K

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


def _taps(cache, layer: int, neurons: bool):
    """(tap keys, weights, the tap's trailing shape, the weights' shape, their names) of the layers below ``layer``"""
    cfg = cache.model.cfg
    if neurons:
        return ([f"blocks.{l}.mlp.hook_post" for l in range(layer)], [cache.model.blocks[l].mlp.W_out for l in range(layer)],
                (cfg.d_mlp,), (cfg.d_mlp, cfg.d_model), ("mlp.hook_post", "[B, T, d_mlp]", "mlp.W_out", "[d_mlp, d_model]"))
    return ([f"blocks.{l}.attn.hook_z" for l in range(layer)], [cache.model.blocks[l].attn.W_O for l in range(layer)],
            (cfg.n_heads, cfg.d_head), (cfg.n_heads, cfg.d_head, cfg.d_model), ("hook_z", "[B, T, H, d_head]", "attn.W_O", "[H, d_head, d_model]"))


def _native_reason(cache, answers: torch.Tensor, layer: int, pos: Optional[int], neurons: bool = False) -> Optional[str]:
    """None when ``pv_head_attribution`` (``neurons``: ``pv_neuron_attribution`` and its top-k form) serves this call, else why
    it does not."""
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
    if neurons:
        if getattr(cfg, "attn_only", False) or not cfg.d_mlp or cfg.d_mlp % 8 != 0:
            return f"d_mlp {getattr(cfg, 'd_mlp', None)} is not a positive multiple of 8"
    elif not (dh in (32, 64) or (64 < dh <= 128 and dh % 8 == 0)):
        return f"d_head {dh} is not 32, 64 or a multiple of 8 in (64, 128]"
    if not 1 <= layer <= MAX_LAYERS:
        return f"{layer} layers below `layer`: the HIP attribution serves 1 .. {MAX_LAYERS}"
    keys, weights, tap_tail, w_shape, (tap_name, tap_form, w_name, w_form) = _taps(cache, layer, neurons)
    scale_key = _scale_key(cache, layer)
    missing = [k for k in keys + [scale_key] if k not in cache.cache_dict]
    if missing:
        return f"the cache lacks {missing[0]}"
    first = cache.cache_dict[keys[0]]
    if not first.is_cuda:
        return "the cache is not on a GPU"
    for k in keys:
        t = cache.cache_dict[k]
        if (t.dtype != torch.bfloat16 or t.dim() != 2 + len(tap_tail) or t.shape != first.shape or t.device != first.device
                or not t.is_contiguous() or tuple(t.shape[2:]) != tap_tail or t.data_ptr() % 16):
            return f"{k} is not a contiguous, 16-byte aligned {tap_form} bf16 tensor on the cache's device"
    if first.numel() * 2 >= 1 << 32:
        return f"a {tap_name} tap holds 4 GiB or more"
    scale = cache.cache_dict[scale_key]
    if (scale.dtype != torch.float32 or scale.shape != (*first.shape[:2], 1) or scale.device != first.device
            or not scale.is_contiguous()):
        return f"{scale_key} is not a contiguous fp32 [B, T, 1] tensor on the cache's device"
    for l, w in enumerate(weights):
        if (w.dtype != torch.bfloat16 or tuple(w.shape) != w_shape or w.device != first.device
                or not w.is_contiguous() or w.data_ptr() % 16):
            return f"blocks.{l}.{w_name} is not a contiguous, 16-byte aligned bf16 {w_form} tensor on the cache's device"
    if not answers.is_floating_point() or answers.shape[-2] == 0:
        return "answers is not a floating-point tensor with at least one row"
    if answers.device != first.device:
        return "answers is not on the cache's device"
    if pos is not None and not 0 <= pos < first.shape[1]:
        return f"pos {pos} is not a token of the cache"
    if torch.is_grad_enabled() and (answers.requires_grad or any(cache.cache_dict[k].requires_grad for k in keys)
                                    or any(w.requires_grad for w in weights)):
        return "autograd is recording"
    if not _native.available():
        return "libpvnative.so is not built"
    return None


def _dispatch(cache, answers: torch.Tensor, layer: int, pos: Optional[int], neurons: bool = False) -> bool:
    global last_run_native, native_fallback_reason
    if _native_mode == "off":
        last_run_native, native_fallback_reason = False, "native_mode == 'off'"
        return False
    reason = _native_reason(cache, answers, layer, pos, neurons)
    if reason is not None and _native_mode == "force":
        raise _native.NativeError(f"native {'neuron' if neurons else 'head'} attribution impossible: {reason}")
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


# ---------------------------------------------------------------------------------------------------------------------------
# by MLP neuron
# ---------------------------------------------------------------------------------------------------------------------------
TopNeurons = collections.namedtuple("TopNeurons", ["values", "layer", "neuron"])
NEURON_SLAB_BYTES = 1 << 30      # most bytes of one [chunk, ..., d_model] slab of the PyTorch path (counted at 4 bytes per element)


def _run_native_neurons(cache, answers: torch.Tensor, layer: int, pos: Optional[int], k: Optional[int] = None, by: int = 0):
    """``pv_neuron_attribution`` (``k`` None: the dense [B, T_out, layer * d_mlp, O]) or ``pv_neuron_attribution_topk`` (values fp32
    and flat indices int32, [B, T_out, O, k] each) on the whole batch, one call per 16 answers."""
    cfg = cache.model.cfg
    taps = [cache.cache_dict[f"blocks.{l}.mlp.hook_post"] for l in range(layer)]
    weights = [cache.model.blocks[l].mlp.W_out.detach() for l in range(layer)]
    scale = cache.cache_dict[_scale_key(cache, layer)]
    B, T, M = taps[0].shape
    per_image = answers.dim() == 3
    O = answers.shape[-2]
    t_out = T if pos is None else 1
    dev = taps[0].device
    answers = answers.detach().to(torch.float32)
    lib = _native.lib()
    p_ptrs = (C.c_void_p * layer)(*[t.data_ptr() for t in taps])
    w_ptrs = (C.c_void_p * layer)(*[w.data_ptr() for w in weights])
    chunks = []
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        for o0 in range(0, O, MAX_ANSWERS):
            a = answers[..., o0:o0 + MAX_ANSWERS, :].contiguous()
            if a.data_ptr() % 16:
                a = a.clone()                                              # (a view at an odd offset: the kernels load 16 bytes)
            n = a.shape[-2]
            ws_bytes = lib.pv_neuron_attribution_workspace_bytes(layer, M, B * n if per_image else n)
            ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
            head = (_native.PV_DTYPE_BF16, p_ptrs, w_ptrs, layer, B, T, -1 if pos is None else int(pos), M, cfg.d_model,
                    scale.data_ptr(), a.data_ptr(), n, 1 if per_image else 0)
            if k is None:
                out = torch.empty((B, t_out, layer * M, n), dtype=torch.float32, device=dev)
                rc = lib.pv_neuron_attribution(*head, out.data_ptr(), ws.data_ptr(), ws_bytes, stream)
                _native.check(rc, "pv_neuron_attribution")
                chunks.append(out)
            else:
                val = torch.empty((B, t_out, n, k), dtype=torch.float32, device=dev)
                idx = torch.empty((B, t_out, n, k), dtype=torch.int32, device=dev)
                rc = lib.pv_neuron_attribution_topk(*head, k, by, val.data_ptr(), idx.data_ptr(), ws.data_ptr(), ws_bytes, stream)
                _native.check(rc, "pv_neuron_attribution_topk")
                chunks.append((val, idx))
    if k is None:
        return chunks[0] if len(chunks) == 1 else torch.cat(chunks, dim=-1)
    if len(chunks) == 1:
        return chunks[0]
    return torch.cat([c[0] for c in chunks], dim=-2), torch.cat([c[1] for c in chunks], dim=-2)


def _run_torch_neurons(cache, answers: torch.Tensor, layer: int, pos: Optional[int]) -> torch.Tensor:
    """The reference's composition -- get_neuron_results, the centring and the division of apply_ln_to_stack, the product with the
    answers -- one layer at a time and in chunks of neurons, so that no more than NEURON_SLAB_BYTES of [chunk, ..., d_model] exist
    at once.  Every element is computed by the operations the helpers apply to it, on tensors laid out as theirs."""
    cfg = cache.model.cfg
    scale = None
    if cfg.normalization_type in ("LN", "LNPre"):
        scale = cache[_scale_key(cache, layer)]
        if pos is not None:
            scale = scale[..., pos:pos + 1, :]
    per_image = answers.dim() == 3
    parts = []
    for l in range(layer):
        post = cache[("post", l, "mlp")]
        if pos is not None:
            post = post[..., pos:pos + 1, :]
        W_out = cache.model.blocks[l].mlp.W_out
        rows = max(1, post.numel() // post.shape[-1])
        chunk = max(1, NEURON_SLAB_BYTES // (rows * cfg.d_model * max(post.element_size(), 4)))
        for n0 in range(0, post.shape[-1], chunk):
            res = (post[..., n0:n0 + chunk, None] * W_out[n0:n0 + chunk]).movedim(-2, 0)          # [chunk, ..., pos, d_model]
            if scale is not None:
                res = (res - res.mean(dim=-1, keepdim=True)) / scale
            parts.append(_times_answers(res, answers, per_image))
    if not parts:
        ref = cache[("resid_pre", 0)]
        lead = ref.shape[:-2] + ((ref.shape[-2] if pos is None else 1),)
        dtype = torch.promote_types(ref.dtype if scale is None else torch.promote_types(ref.dtype, scale.dtype), answers.dtype)
        return torch.zeros((*lead, 0, answers.shape[-2]), dtype=dtype, device=ref.device)
    return torch.cat(parts, dim=0).movedim(0, -2)


def topk_order(attr: torch.Tensor, k: int, by: str = "value"):
    """``(values, flat index)``, ``[..., O, k]`` each, of a dense ``[..., C, O]`` attribution: per answer the ``k`` components with the
    largest key -- the value, or its magnitude with ``by="abs"`` -- where keys compare as floats (-0 equals +0), a NaN is greater
    than everything and ties go to the lowest index.  A stable descending sort has exactly that order; ``torch.topk`` leaves the
    order of ties open."""
    v = attr.movedim(-2, -1)                                                   # [..., O, C]
    order = torch.sort(v.abs() if by == "abs" else v, dim=-1, descending=True, stable=True).indices[..., :k]
    return torch.gather(v, -1, order), order


def _check_neuron_call(cache, answers: torch.Tensor, layer: Optional[int], pos: Optional[int]):
    cfg = cache.model.cfg
    layer = _resolve_layer(cache, layer)
    if answers.dim() not in (2, 3) or answers.shape[-1] != cfg.d_model:
        raise ValueError(f"answers must be [O, d_model] or [B, O, d_model] with d_model = {cfg.d_model}, not {tuple(answers.shape)}")
    if answers.dim() == 3:
        if not cache.has_batch_dim:
            raise ValueError("answers per image need a cache with a batch dimension")
        n_images = cache[("post", 0, "mlp")].shape[0]
        if answers.shape[0] != n_images:
            raise ValueError(f"answers hold {answers.shape[0]} images, the cache {n_images}")
    return layer, (None if pos is None else int(pos))


def neuron_logit_attribution(cache, answers: torch.Tensor, layer: Optional[int] = None, pos: Optional[int] = None,
                             return_labels: bool = True):
    """``(attr [B, T, layer * d_mlp, O], labels)``: what every MLP neuron of the layers below ``layer`` writes along each answer
    direction after the LayerNorm scaling of the layer it feeds -- ``einsum(cache.stack_neuron_results(layer, apply_ln=True),
    answers)`` without the ``[layer * d_mlp, B, T, d_model]`` stack; ``[B, 1, layer * d_mlp, O]`` with ``pos``.  ``answers``:
    ``[O, d_model]`` shared, or ``[B, O, d_model]`` per image.  Labels ``"L{l}N{n}"`` as in ``stack_neuron_results``.  The dense
    result is large (B T layer d_mlp O floats): over every token, ``top_neuron_logit_attribution`` is the form to use."""
    layer, pos = _check_neuron_call(cache, answers, layer, pos)
    labels = [f"L{l}N{n}" for l in range(layer) for n in range(cache.model.cfg.d_mlp)] if return_labels else None
    if _dispatch(cache, answers, layer, pos, neurons=True):
        attr = _run_native_neurons(cache, answers, layer, pos).to(torch.promote_types(torch.float32, answers.dtype))
    else:
        attr = _run_torch_neurons(cache, answers, layer, pos)
    return (attr, labels) if return_labels else attr


def top_neuron_logit_attribution(cache, answers: torch.Tensor, k: int, layer: Optional[int] = None, pos: Optional[int] = None,
                                 by: str = "value") -> TopNeurons:
    """``TopNeurons(values, layer, neuron)``, ``[B, T, O, k]`` each (``[B, 1, O, k]`` with ``pos``): per token and answer the ``k``
    neurons of the layers below ``layer`` whose ``neuron_logit_attribution`` is largest (``by="value"``) or largest in magnitude
    (``by="abs"``; ``values`` stay signed), sorted from the largest on.  Keys compare as floats, a NaN counts as the greatest
    and ties go to the lower ``layer * d_mlp + neuron``.  On the HIP path the dense tensor is never stored
    (``pv_neuron_attribution_topk``, ``k <= 256``); the PyTorch path orders the dense result."""
    layer, pos = _check_neuron_call(cache, answers, layer, pos)
    if by not in ("value", "abs"):
        raise ValueError(f"by must be 'value' or 'abs', not {by!r}")
    M = cache.model.cfg.d_mlp
    k = int(k)
    if not 1 <= k <= layer * M:
        raise ValueError(f"k = {k} is outside 1 .. layer * d_mlp = {layer * M}")
    native = _dispatch(cache, answers, layer, pos, neurons=True)
    if native and k > MAX_TOPK:
        global last_run_native, native_fallback_reason
        reason = f"k = {k} is above {MAX_TOPK}, the most the HIP top-k returns"
        if _native_mode == "force":
            raise _native.NativeError(f"native neuron attribution impossible: {reason}")
        native, last_run_native, native_fallback_reason = False, False, reason
    if native:
        values, flat = _run_native_neurons(cache, answers, layer, pos, k=k, by=1 if by == "abs" else 0)
        values, flat = values.to(torch.promote_types(torch.float32, answers.dtype)), flat.long()
    else:
        values, flat = topk_order(_run_torch_neurons(cache, answers, layer, pos), k, by)
    return TopNeurons(values, flat // M, flat % M)
