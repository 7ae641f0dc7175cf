"""Patch-level logit lens (the reference's prisma_tools/logit_lens.py) on the cached residual stream.

    directions, labels = get_patch_logit_directions(cache, all_answers)          # [B, T, S, O]
    table = get_patch_logit_dictionary((directions, labels), batch_idx=0)

    top_idx, top_logit, rank, labels = patch_logit_top(cache, all_answers, rank_index=label)   # [B, T, S] each, no [B, T, S, O]
    table = patch_logit_dictionary(cache, all_answers, batch_idx=0, rank_label=label)

On a bf16 model whose cache lives on the GPU both forms run in ``pv_logit_lens`` (csrc/lens.hip): one pass over the residual
taps where they lie, centring applied to the fp32 sums, no stack copy and no normalised intermediate.  ``all_answers`` is
multiplied as bf16 there: answers that are not bf16-representable are rounded once.  Everything else -- fp32
models, CPU caches, caches without a batch dimension -- runs the three reference steps through ``ActivationCache``.  Which of
the two ran is in ``last_run_native`` / ``native_fallback_reason``; ``use_native(True)`` turns a fallback into an error.

The reference's plotting functions (visualization/patch_level_logit_lens.py) are not part of this package, and neither is its
ImageNet name table: pass ``class_names`` (a sequence indexed by class) where names are wanted.
"""
from __future__ import annotations

import ctypes as C
from collections import defaultdict
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

from . import _native

last_run_native: bool = False
native_fallback_reason: Optional[str] = None
_native_mode = "auto"            # "auto" | "off" | "force"


def use_native(mode: Union[bool, str, None]) -> None:
    """True/"force": raise unless the HIP path can run; False/"off": always PyTorch; None/"auto": the HIP path where it applies."""
    global _native_mode
    mode = {True: "force", False: "off", None: "auto"}.get(mode, mode)
    assert mode in ("auto", "off", "force")
    _native_mode = mode


def _stack_entries(cache, incl_mid: bool) -> Tuple[List[str], List[str]]:
    """(cache keys, labels) of ``cache.accumulated_resid(layer=-1, incl_mid=incl_mid)``, in its order."""
    from .utils import get_act_name
    n_layers = cache.model.cfg.n_layers
    keys, labels = [], []
    for l in range(n_layers):
        keys.append(get_act_name("resid_pre", l))
        labels.append(f"{l}_pre")
        if incl_mid:
            keys.append(get_act_name("resid_mid", l))
            labels.append(f"{l}_mid")
    keys.append(get_act_name("resid_post", n_layers - 1))
    labels.append("final_post")
    return keys, labels


def _native_reason(cache, all_answers: torch.Tensor, keys: List[str]) -> Optional[str]:
    """None when ``pv_logit_lens`` serves this call, else why it does not."""
    cfg = cache.model.cfg
    if not cache.has_batch_dim:
        return "the cache has no batch dimension"
    if cfg.normalization_type != "LN":
        return f"normalization_type is {cfg.normalization_type!r}, not 'LN'"
    if cfg.dtype != torch.bfloat16:
        return f"the model is {cfg.dtype}, the HIP lens serves bf16"
    if cfg.d_model % 8 != 0:
        return "d_model is not a multiple of 8"
    if len(keys) > 128:
        return "more than 128 stack entries"
    missing = [k for k in keys + ["ln_final.hook_scale"] if k not in cache.cache_dict]
    if missing:
        return f"the cache lacks {missing[0]}"
    first = cache.cache_dict[keys[0]]
    if not first.is_cuda:
        return "the cache is not on a GPU"
    for k in keys:
        t = cache.cache_dict[k]
        if (t.dtype != torch.bfloat16 or t.dim() != 3 or t.shape != first.shape or t.device != first.device
                or not t.is_contiguous() or t.shape[-1] != cfg.d_model):
            return f"{k} is not a contiguous [B, T, d_model] bf16 tensor on the cache's device"
    scale = cache.cache_dict["ln_final.hook_scale"]
    if (scale.dtype != torch.float32 or scale.shape != (*first.shape[:2], 1) or scale.device != first.device
            or not scale.is_contiguous()):
        return "ln_final.hook_scale is not a contiguous fp32 [B, T, 1] tensor on the cache's device"
    if all_answers.dim() != 2 or all_answers.shape[1] != cfg.d_model or all_answers.device != first.device:
        return "all_answers is not an [O, d_model] tensor on the cache's device"
    if not all_answers.is_floating_point():
        return "all_answers is not a floating-point tensor"
    if torch.is_grad_enabled() and (all_answers.requires_grad or any(cache.cache_dict[k].requires_grad for k in keys)):
        return "autograd is recording"
    if not _native.available():
        return "libpvnative.so is not built"
    return None


def _dispatch(cache, all_answers: torch.Tensor, keys: List[str]) -> bool:
    global last_run_native, native_fallback_reason
    if _native_mode == "off":
        last_run_native, native_fallback_reason = False, "native_mode == 'off'"
        return False
    reason = _native_reason(cache, all_answers, keys)
    if reason is not None and _native_mode == "force":
        raise _native.NativeError(f"native logit lens impossible: {reason}")
    last_run_native, native_fallback_reason = reason is None, reason
    return reason is None


def _result_dtype(cache, all_answers: torch.Tensor, keys: List[str]) -> torch.dtype:
    """dtype of the reference's result: the stack promoted by the division with hook_scale, then by the answers."""
    stack_dtype = torch.promote_types(cache.cache_dict[keys[0]].dtype, cache.cache_dict["ln_final.hook_scale"].dtype) \
        if cache.model.cfg.normalization_type in ("LN", "LNPre") else cache.cache_dict[keys[0]].dtype
    return torch.promote_types(stack_dtype, all_answers.dtype)


def _run_native(cache, all_answers: torch.Tensor, keys: List[str], want_directions: bool, want_top: bool,
                rank_index: Optional[int], batch_idx: Optional[int] = None):
    """One ``pv_logit_lens`` call on the whole batch, or on image ``batch_idx`` alone."""
    taps = [cache.cache_dict[k] for k in keys]
    scale = cache.cache_dict["ln_final.hook_scale"]
    if batch_idx is not None:
        b = range(taps[0].shape[0])[batch_idx]
        taps = [t[b:b + 1] for t in taps]
        scale = scale[b:b + 1]
    B, T, d = taps[0].shape
    N, S, O = B * T, len(taps), all_answers.shape[0]
    dev = taps[0].device
    answers = all_answers.detach().to(torch.bfloat16).contiguous()
    lib = _native.lib()
    with torch.cuda.device(dev):
        ws_bytes = lib.pv_logit_lens_workspace_bytes(N, S, d, O)
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
        directions = torch.empty((B, T, S, O), dtype=torch.float32, device=dev) if want_directions else None
        top_idx = torch.empty((B, T, S), dtype=torch.int32, device=dev) if want_top else None
        top_logit = torch.empty((B, T, S), dtype=torch.float32, device=dev) if want_top else None
        rank = torch.empty((B, T, S), dtype=torch.int32, device=dev) if (want_top and rank_index is not None) else None
        ptrs = (C.c_void_p * S)(*[t.data_ptr() for t in taps])
        ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
        rc = lib.pv_logit_lens(_native.PV_DTYPE_BF16, ptrs, S, N, d, scale.data_ptr(), answers.data_ptr(), O, ptr(directions),
                               ptr(top_idx), ptr(top_logit), -1 if rank_index is None else int(rank_index), ptr(rank),
                               ws.data_ptr(), ws_bytes, torch.cuda.current_stream(dev).cuda_stream)
        _native.check(rc, "pv_logit_lens")
        # (the stream orders the kernels before any later use or reuse of `ws` / `answers` memory: the caching allocator hands
        # a freed block to work on the same stream only)
    return directions, top_idx, top_logit, rank


def _directions_torch(cache, all_answers: torch.Tensor, incl_mid: bool):
    """logit_lens.py:36-45, with the operands of the product brought to their common dtype first (torch.einsum takes no mix)."""
    stack, labels = cache.accumulated_resid(layer=-1, incl_mid=incl_mid, return_labels=True)
    scaled = cache.apply_ln_to_stack(stack, layer=-1)
    dtype = torch.promote_types(scaled.dtype, all_answers.dtype)
    result = torch.einsum("l...d,od->l...o", scaled.to(dtype), all_answers.to(dtype))
    return result.movedim(0, -2), labels


def get_patch_logit_directions(cache, all_answers: torch.Tensor, incl_mid: bool = False, return_labels: bool = True) -> tuple:
    """The residual stream at the input of every layer and after the last, centred, divided by the cached ``ln_final.hook_scale``
    and multiplied with ``all_answers [O, d_model]``: ``(result [B, T, S, O], labels)`` (logit_lens.py:20-45; like the
    reference, ``return_labels`` does not change what is returned)."""
    keys, labels = _stack_entries(cache, incl_mid)
    if _dispatch(cache, all_answers, keys):
        directions, _, _, _ = _run_native(cache, all_answers, keys, True, False, None)
        return directions.to(_result_dtype(cache, all_answers, keys)), labels
    return _directions_torch(cache, all_answers, incl_mid)


def _top_of(directions: torch.Tensor, rank_index: Optional[int]):
    """Top-1 index, its logit and the label's rank over the last dimension: ties go to the lowest index (torch.argmax), the
    rank counts larger logits plus equal ones at a lower index; rows whose label logit is NaN get rank -1."""
    top_idx = directions.argmax(dim=-1)
    top_logit = directions.gather(-1, top_idx[..., None])[..., 0]
    rank = None
    if rank_index is not None:
        lab = directions[..., rank_index:rank_index + 1]
        lower = torch.arange(directions.shape[-1], device=directions.device) < rank_index
        rank = ((directions > lab) | ((directions == lab) & lower)).sum(dim=-1)
        rank = torch.where(torch.isnan(lab[..., 0]), torch.full_like(rank, -1), rank)
    return top_idx, top_logit, rank


def patch_logit_top(cache, all_answers: torch.Tensor, incl_mid: bool = False, rank_index: Optional[int] = None,
                    return_labels: bool = True):
    """``(top_idx, top_logit, rank | None, labels)``, ``[B, T, S]`` each: what ``get_patch_logit_dictionary`` reads off the
    directions, for every image at once and (on the HIP path) without materialising ``[B, T, S, O]``."""
    keys, labels = _stack_entries(cache, incl_mid)
    if rank_index is not None and not 0 <= int(rank_index) < all_answers.shape[0]:
        raise IndexError(f"rank_index {rank_index} is not a row of all_answers ({all_answers.shape[0]})")
    if _dispatch(cache, all_answers, keys):
        _, top_idx, top_logit, rank = _run_native(cache, all_answers, keys, False, True, rank_index)
        top_idx = top_idx.long()
        top_logit = top_logit.to(_result_dtype(cache, all_answers, keys))
        rank = None if rank is None else rank.long()
    else:
        directions, labels = _directions_torch(cache, all_answers, incl_mid)
        top_idx, top_logit, rank = _top_of(directions, rank_index)
    return (top_idx, top_logit, rank, labels) if return_labels else (top_idx, top_logit, rank)


def _rank_column(rank_label: Union[int, str, None], class_names: Optional[Sequence[str]]) -> Optional[int]:
    if rank_label is None:
        return None
    if isinstance(rank_label, str):
        if class_names is None:
            raise ValueError("a rank_label given by name needs class_names to look it up in")
        return list(class_names).index(rank_label)
    return int(rank_label)


def _dictionary(top_idx: torch.Tensor, top_logit: torch.Tensor, rank: Optional[torch.Tensor],
                class_names: Optional[Sequence[str]]) -> Dict[int, List[tuple]]:
    """[T, S] tensors -> {patch: [(logit, class name, class index[, rank]) per stack entry]} with one transfer each."""
    idx, logit = top_idx.tolist(), top_logit.tolist()
    ranks = None if rank is None else rank.tolist()
    name = (lambda i: str(i)) if class_names is None else (lambda i: class_names[i])
    table: Dict[int, List[tuple]] = defaultdict(list)
    for t in range(len(idx)):
        for s in range(len(idx[t])):
            cell = (logit[t][s], name(idx[t][s]), idx[t][s])
            table[t].append(cell + (ranks[t][s],) if ranks is not None else cell)
    return table


def get_patch_logit_dictionary(patch_logit_directions: Union[torch.Tensor, Tuple[torch.Tensor, ...]], batch_idx: int = 0,
                               rank_label: Union[int, str, None] = None,
                               class_names: Optional[Sequence[str]] = None) -> Dict[int, List[tuple]]:
    """``{patch: [(logit, class name, class index[, rank]) per stack entry]}`` for image ``batch_idx`` (logit_lens.py:47-89), from
    directions ``[B, T, S, O]`` or the ``(directions, labels)`` pair.  One argmax / gather / count over ``[T, S, O]`` instead of a
    softmax per cell.  ``class_names``: a sequence indexed by class (absent: ``str(index)``); ``rank_label``: a column, or a name
    to look up in ``class_names``.  The rank counts larger logits plus equal ones at a lower index."""
    if isinstance(patch_logit_directions, tuple):
        patch_logit_directions = patch_logit_directions[0]
    top_idx, top_logit, rank = _top_of(patch_logit_directions[batch_idx], _rank_column(rank_label, class_names))
    return _dictionary(top_idx, top_logit, rank, class_names)


def patch_logit_dictionary(cache, all_answers: torch.Tensor, batch_idx: int = 0, incl_mid: bool = False,
                           rank_label: Union[int, str, None] = None,
                           class_names: Optional[Sequence[str]] = None) -> Dict[int, List[tuple]]:
    """``get_patch_logit_dictionary(get_patch_logit_directions(cache, all_answers, incl_mid), batch_idx, ...)`` without the
    directions: on the HIP path the top form of ``pv_logit_lens`` on image ``batch_idx`` alone."""
    rank_index = _rank_column(rank_label, class_names)
    keys, _ = _stack_entries(cache, incl_mid)
    if _dispatch(cache, all_answers, keys):
        _, top_idx, top_logit, rank = _run_native(cache, all_answers, keys, False, True, rank_index, batch_idx=batch_idx)
        return _dictionary(top_idx[0], top_logit[0], None if rank is None else rank[0], class_names)
    directions, _ = _directions_torch(cache, all_answers, incl_mid)
    top_idx, top_logit, rank = _top_of(directions[batch_idx] if cache.has_batch_dim else directions, rank_index)
    return _dictionary(top_idx, top_logit, rank, class_names)
