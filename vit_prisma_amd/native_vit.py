"""Host driver of the native (HIP) tapped ViT forward: plan, weight shadow, workspace, and the
HBM tap arena that backs ActivationCache tensors.

PyTorch is plumbing here: it owns device memory and streams; all arithmetic happens in
libpvnative.so behind the C ABI of include/pv_native.h.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import torch

from . import _native as N
from .split_plan import EXIT, KIND
from .tap_plan import TapSpec, final_residual_name, head_out_shape, hook_order, pooling_mode, tap_spec

_ALIGN = 256
_ESIZE = {torch.float32: 4, torch.bfloat16: 2, torch.float16: 2}


def _use_count(t: torch.Tensor) -> int:
    return torch._C._storage_Use_Count(t.untyped_storage()._cdata)


class TapArena:
    """Ring of HBM slabs that tap stores go to.  One ``run_with_cache`` call takes ONE slab and
    carves every cached activation out of it as a tensor view, so the reference's lifetime
    semantics hold (a cache entry stays valid for as long as the user holds it, cf.
    hooked_root_module.py:312-316 where entries alias live activations): a slab is handed out
    again only when the storage use-count shows no outstanding view; if every slab is still
    referenced a new one is allocated (spill), never overwritten.
    """

    def __init__(self, device: torch.device, max_slabs: int = 4):
        self.device = device
        self.max_slabs = max_slabs
        self._slabs: List[Tuple[torch.Tensor, int]] = []   # (uint8 tensor, baseline use-count)
        self.n_alloc = 0
        self.n_reuse = 0

    def acquire(self, nbytes: int) -> torch.Tensor:
        nbytes = max(int(nbytes), _ALIGN)
        for slab, base in self._slabs:
            if slab.numel() >= nbytes and _use_count(slab) <= base:
                self.n_reuse += 1
                return slab
        slab = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        base = _use_count(slab)
        self.n_alloc += 1
        # keep the ring bounded: evict free slabs that are too small, oldest first
        free_small = [i for i, (s, b) in enumerate(self._slabs) if _use_count(s) <= b and s.numel() < nbytes]
        for i in reversed(free_small):
            del self._slabs[i]
        if len(self._slabs) < self.max_slabs:
            self._slabs.append((slab, base))
        return slab

    def bytes_held(self) -> int:
        return sum(s.numel() for s, _ in self._slabs)


class PinnedMirror:
    """Pinned host slab for ``device='cpu'`` requests: ONE async D2H copy of the whole tap slab on
    a side stream and one event sync, instead of one synchronous copy per hook point."""

    def __init__(self):
        self._buf: Optional[torch.Tensor] = None
        self._stream: Optional[torch.cuda.Stream] = None

    def copy_from(self, slab: torch.Tensor, nbytes: int) -> torch.Tensor:
        # a fresh pinned buffer per call keeps cache lifetime semantics (the user owns the views)
        host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        if self._stream is None:
            self._stream = torch.cuda.Stream(device=slab.device)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(slab.device))
        with torch.cuda.stream(self._stream):
            self._stream.wait_event(ev)
            host.copy_(slab[:nbytes], non_blocking=True)
            done = torch.cuda.Event()
            done.record(self._stream)
        done.synchronize()
        return host


_STRIDES: Dict[Tuple[int, ...], Tuple[int, ...]] = {}


def _contiguous_strides(shape: Tuple[int, ...]) -> Tuple[int, ...]:
    st = _STRIDES.get(shape)
    if st is None:
        acc, rev = 1, []
        for dim in reversed(shape):
            rev.append(acc)
            acc *= dim
        st = _STRIDES[shape] = tuple(reversed(rev))
    return st


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


class NativeViT:
    """Owns one pv_vit_plan for one (config, dtype, device)."""

    def __init__(self, cfg, n_tokens: int, device: torch.device):
        if cfg.dtype not in (torch.float32, torch.bfloat16):
            raise N.NativeError(f"native path supports fp32 / bf16 storage, not {cfg.dtype}")
        self.cfg = cfg
        self.device = torch.device(device)
        self.n_tokens = n_tokens
        self.lib = N.lib()
        self._plan = C.c_void_p()
        self._create_plan()
        self._shadow: Optional[torch.Tensor] = None
        self._weights_key = None
        self._frozen = False
        self._keepalive = None
        self._workspace: Optional[torch.Tensor] = None
        self.arena = TapArena(self.device)
        self.mirror = PinnedMirror()
        self.n_forward = 0
        self.n_repack = 0
        self._param_slots = None
        # host-side plans of repeated calls: (names, batch, segment) -> tap layout in the slab + how each cache entry is viewed; per
        # slab base the ctypes tap array.  A 214-tap call spent 1.7 ms on the host rebuilding them (a bs = 32 forward takes 0.45 ms)
        self._layouts: Dict[tuple, tuple] = {}
        self._tap_arrays: Dict[tuple, object] = {}

    def _create_plan(self) -> None:
        cfg = self.cfg
        desc = N.VitDesc(
            n_layers=cfg.n_layers, d_model=cfg.d_model, n_heads=cfg.n_heads, d_head=cfg.d_head,
            d_mlp=cfg.d_mlp, n_channels=cfg.n_channels, patch_size=cfg.patch_size,
            image_size=cfg.image_size, n_tokens=self.n_tokens, n_classes=cfg.n_classes,
            use_cls_token=int(bool(cfg.use_cls_token)), layer_norm_pre=int(bool(cfg.layer_norm_pre)),
            has_head=int(cfg.return_type != "pre_logits"), normalize_output=int(bool(cfg.normalize_output)),
            activation=N.PV_ACT[cfg.activation_name],
            dtype=N.PV_DTYPE_BF16 if cfg.dtype == torch.bfloat16 else N.PV_DTYPE_F32,
            eps=float(cfg.eps),
            attn_scale=float(cfg.d_head ** 0.5) if cfg.use_attn_scale else 1.0,
            pooling=pooling_mode(cfg))
        N.check(self.lib.pv_vit_plan_create(C.byref(desc), C.byref(self._plan)), "pv_vit_plan_create")

    def __del__(self):
        try:
            if getattr(self, "_plan", None) is not None and self._plan.value:
                self.lib.pv_vit_plan_destroy(self._plan)
                self._plan = C.c_void_p()
        except Exception:
            pass

    # ---- weights ---------------------------------------------------------------------------
    @staticmethod
    def supported(cfg, n_tokens: int) -> Optional[str]:
        """None if the native plan supports this config, else the reason it does not."""
        if cfg.dtype not in (torch.float32, torch.bfloat16):
            return f"dtype {cfg.dtype}"
        if cfg.normalization_type != "LN":
            return f"normalization_type {cfg.normalization_type}"
        if cfg.activation_name not in N.PV_ACT:
            return f"activation {cfg.activation_name}"
        if cfg.classification_type not in ("cls", "gaap"):
            return "classification_type"
        if pooling_mode(cfg) == N.PV_POOL_CLS_MEAN and cfg.return_type != "pre_logits":
            # [B, d_model, 2] @ W_H: no entry of the reference's registry has it; the plan builds the concatenation without a head only
            return "classification_type: the dino-vitb concatenation (cls, mean of patches) with a head stays on the PyTorch path"
        if getattr(cfg, "is_video_transformer", False) or getattr(cfg, "use_bert_block", False) or cfg.attn_only:
            return "architecture variant"
        if cfg.d_model % 8 or cfg.d_mlp % 8 or cfg.d_model > 2048:
            return "d_model/d_mlp alignment"
        if n_tokens > N.ATTN_MAX_TOKENS or not N.attention_head_supported(cfg.d_head):
            return "attention shape"
        if pooling_mode(cfg) == N.PV_POOL_CLS_MEAN and n_tokens < 2:
            return "classification_type: no patch token to average"
        if cfg.attn_dropout_rate or cfg.mlp_dropout_rate:
            return None  # dropout is the identity in eval mode; training mode is checked by the caller
        return None

    def _borrow(self, keep: List[torch.Tensor]):
        """P(tensor) -> its device pointer, the (contiguous) tensor kept alive in ``keep``."""
        cfg = self.cfg

        def P(t: Optional[torch.Tensor]) -> Optional[int]:
            if t is None:
                return None
            t = t.detach()
            if t.device != self.device or t.dtype != cfg.dtype:
                raise N.NativeError(f"parameter on {t.device}/{t.dtype}, plan is {self.device}/{cfg.dtype}")
            if not t.is_contiguous():
                t = t.contiguous()
            keep.append(t)
            return t.data_ptr()
        return P

    def _collect_layers(self, model, P):
        L = (N.VitLayerWeights * max(self.cfg.n_layers, 1))()
        for i, blk in enumerate(model.blocks):
            a, m = blk.attn, blk.mlp
            L[i] = N.VitLayerWeights(
                ln1_w=P(blk.ln1.w), ln1_b=P(blk.ln1.b), W_Q=P(a.W_Q), W_K=P(a.W_K), W_V=P(a.W_V),
                b_Q=P(a.b_Q), b_K=P(a.b_K), b_V=P(a.b_V), W_O=P(a.W_O), b_O=P(a.b_O),
                ln2_w=P(blk.ln2.w), ln2_b=P(blk.ln2.b), W_in=P(m.W_in), b_in=P(m.b_in),
                W_out=P(m.W_out), b_out=P(m.b_out))
        return L

    def _collect(self, model) -> Tuple[N.VitWeights, list]:
        cfg = self.cfg
        keep: List[torch.Tensor] = []
        P = self._borrow(keep)
        L = self._collect_layers(model, P)
        has_head = cfg.return_type != "pre_logits"
        W = N.VitWeights(
            cls_token=P(model.cls_token) if cfg.use_cls_token else None,
            conv_w=P(model.embed.proj.weight), conv_b=P(model.embed.proj.bias),
            W_pos=P(model.pos_embed.W_pos),
            ln_pre_w=P(model.ln_pre.w) if cfg.layer_norm_pre else None,
            ln_pre_b=P(model.ln_pre.b) if cfg.layer_norm_pre else None,
            ln_final_w=P(model.ln_final.w), ln_final_b=P(model.ln_final.b),
            W_H=P(model.head.W_H) if has_head else None, b_H=P(model.head.b_H) if has_head else None,
            layers=C.cast(L, C.POINTER(N.VitLayerWeights)))
        return W, [keep, L]

    def _plan_slots(self, model) -> list:
        """(module, parameter name) of exactly the parameters the plan borrows (what ``_collect`` reads) -- the one list both the
        change detection and the key stored after a repack are built from (round-5 advisor: the stored key came from
        ``model.parameters()``, a different walk -- tied parameters de-duplicated, spliced modules included -- so after one real
        repack the two could never match again and every forward repacked the whole shadow)."""
        cfg = self.cfg
        slots = self._block_slots(model)
        if cfg.use_cls_token:
            slots.append((model, "cls_token"))
        slots += [(model.embed.proj, "weight"), (model.embed.proj, "bias"), (model.pos_embed, "W_pos"), (model.ln_final, "w"), (model.ln_final, "b")]
        if cfg.layer_norm_pre:
            slots += [(model.ln_pre, "w"), (model.ln_pre, "b")]
        if cfg.return_type != "pre_logits":
            slots += [(model.head, "W_H"), (model.head, "b_H")]
        return slots

    @staticmethod
    def _block_slots(model) -> list:
        slots = []
        for blk in model.blocks:
            slots += [(blk.ln1, "w"), (blk.ln1, "b"), (blk.ln2, "w"), (blk.ln2, "b")]
            slots += [(blk.attn, n) for n in ("W_Q", "W_K", "W_V", "b_Q", "b_K", "b_V", "W_O", "b_O")]
            slots += [(blk.mlp, n) for n in ("W_in", "b_in", "W_out", "b_out")]
        return slots

    @staticmethod
    def _slots_key(slots) -> tuple:
        return tuple((p.data_ptr(), p._version) for p in (m._parameters.get(n) for m, n in slots) if p is not None)

    def sync_weights(self, model, force: bool = False) -> None:
        """(Re)pack the MFMA-layout weight shadow when parameters changed (data_ptr / _version of
        any parameter) -- or unconditionally with force=True (edits through ``.data`` are invisible
        to the version counter; ``HookedViT.invalidate_native_weights()`` forces a repack)."""
        if self._frozen and not force and self._weights_key is not None:
            return
        # (every call pays this check: walk the (module, name) slots of the parameters the plan borrows, found once, instead of
        # model.parameters() -- 0.5 ms of module-tree traversal per call, which is what a small-batch forward costs on the GPU; a
        # Parameter object replaced in its slot is seen; a block object replaced in model.blocks is seen by the identity of the list)
        slots = self._param_slots
        blocks = tuple(model.blocks)
        if slots is None or slots[0] is not model or slots[2] != blocks:
            slots = self._param_slots = (model, self._plan_slots(model), blocks)
        key = self._slots_key(slots[1])
        if not force and key == self._weights_key:
            return
        W, keep = self._collect(model)
        nbytes = self.lib.pv_vit_shadow_bytes(self._plan)
        if self._shadow is None or self._shadow.numel() < nbytes:
            self._shadow = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self._set_weights(W, nbytes, stream)
        self._keepalive = keep
        self._weights_key = key
        self.n_repack += 1

    def _set_weights(self, W, nbytes: int, stream: int) -> None:
        N.check(self.lib.pv_vit_plan_set_weights(self._plan, C.byref(W), self._shadow.data_ptr(), nbytes, stream),
                "pv_vit_plan_set_weights")

    def freeze_weights(self, frozen: bool = True) -> None:
        self._frozen = frozen

    # ---- forward ---------------------------------------------------------------------------
    def _get_workspace(self, batch: int) -> torch.Tensor:
        need = self.lib.pv_vit_workspace_bytes(self._plan, batch)
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = None
            self._workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._workspace

    def _check_input(self, images: torch.Tensor) -> torch.Tensor:
        """The model input as the plan reads it (dtype, layout); raises on a shape the plan was not built for."""
        cfg = self.cfg
        if images.dtype != cfg.dtype:
            images = images.to(cfg.dtype)
        images = images.contiguous()
        if tuple(images.shape[1:]) != (cfg.n_channels, cfg.image_size, cfg.image_size):
            raise ValueError(f"expected images [B,{cfg.n_channels},{cfg.image_size},{cfg.image_size}], got {tuple(images.shape)}")
        return images

    def _launch_full(self, inp: torch.Tensor, B: int, n_blocks: int, run_head: bool, taps, n_taps: int, ws: torch.Tensor,
                     out_ptr: Optional[int], stream: int) -> None:
        """The forward from the model input (no resumed segment)."""
        N.check(self.lib.pv_vit_forward(self._plan, inp.data_ptr(), B, n_blocks, int(run_head), taps, n_taps,
                                        ws.data_ptr(), ws.numel(), out_ptr, stream),
                "pv_vit_forward")

    def _pos_embed_view(self, model, B: int) -> torch.Tensor:
        """hook_pos_embed: stride-0 broadcast view of W_pos, as in position_embedding.py:36-38"""
        return model.pos_embed.W_pos.detach().unsqueeze(0).expand(B, -1, -1)

    def forward(self, model, images: Optional[torch.Tensor], names: Sequence[str], n_blocks: int, run_head: bool,
                cache_device=None, remove_batch_dim: bool = False, first_block: int = 0,
                resid_in: Optional[torch.Tensor] = None, entry_stage: int = 0, exit_stage: int = 0,
                act_in: Sequence[torch.Tensor] = (),
                tap_dst: Optional[Dict[str, torch.Tensor]] = None) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
        """Runs the tapped forward.  ``names``: requested HookPoint names in firing order.
        ``tap_dst`` {name: tensor}: the caller's OWN destination for a requested activation (the activation store's buffer
        slice): the producing kernel stores straight into it and the cache entry IS that tensor -- taken only when the tensor
        is exactly what the tap writes (device, dtype, shape, contiguous, 256-byte aligned); otherwise the entry comes out of
        the arena as usual and the caller copies.
        With ``resid_in`` ([B, T, d_model]) the forward is RESUMED at block ``first_block`` from that residual
        (``images`` is ignored, names of earlier stages must not be requested).  Positions inside a block
        (``entry_stage`` / ``exit_stage``, pv_vit_forward_stage): the PV_STAGE_* numbers, named and described by the two tables of
        split_plan (``ENTRY`` .. ``MLP_POST``; ``EXIT[stage]``).  A segment that exits at a stage runs block ``n_blocks`` up to it; one
        that enters at a stage gets the residual stream the rest of the block adds to (``EXIT[stage].carried``) in ``resid_in`` and
        the (hook-edited) activations of the stage in ``act_in``: the kinds of ``EXIT[stage].acts``, fp32 at the LayerNorm stages.
        Returns (model_out, {name: tensor}); for an exit inside a block model_out is the stage's first activation
        (``EXIT[stage].acts[0]``; behind the attention half, which hands on no activation, hook_resid_mid)."""
        entry_stage, exit_stage = int(entry_stage), int(exit_stage)
        cfg = self.cfg
        T = self.n_tokens
        if resid_in is not None:
            if resid_in.device != self.device:
                raise N.NativeError(f"residual on {resid_in.device}, model on {self.device}")
            if tuple(resid_in.shape[1:]) != (T, cfg.d_model):
                raise ValueError(f"expected a residual [B,{T},{cfg.d_model}], got {tuple(resid_in.shape)}")
            resid_in = resid_in.to(cfg.dtype).contiguous()
            images = resid_in                       # (only .element_size() / batch are read below)
            B = resid_in.shape[0]
        else:
            if images.device != self.device:
                raise N.NativeError(f"input on {images.device}, model on {self.device}")
            images = self._check_input(images)
            B = images.shape[0]
        self.sync_weights(model)

        lkey = None if tap_dst else (tuple(names), B, n_blocks, bool(run_head), exit_stage)
        layout = self._layouts.get(lkey) if lkey is not None else None
        if layout is not None:
            specs, out_name = layout[0], layout[1]
        else:
            specs = {n: tap_spec(n, cfg, B, T) for n in names}
        out_name = None if layout is None else out_name
        if layout is None and not run_head:
            ex = EXIT[exit_stage]
            out_name = f"blocks.{n_blocks}.{KIND[(ex.acts or ex.taps)[0]].sub}" if exit_stage else final_residual_name(cfg, n_blocks)
            if out_name not in specs:
                specs[out_name] = tap_spec(out_name, cfg, B, T)
        acts = []
        act_dtype = torch.float32 if EXIT[entry_stage].ln else cfg.dtype      # (the LayerNorm points carry fp32 in either mode)
        for t in act_in:
            if t.device != self.device:
                raise N.NativeError(f"activation on {t.device}, model on {self.device}")
            acts.append(t.to(act_dtype).contiguous())
        want_acts = len(EXIT[entry_stage].acts)
        if len(acts) != want_acts:
            raise ValueError(f"entry_stage {entry_stage} takes {want_acts} activation tensors, got {len(acts)}")
        # unique buffers -> slab offsets
        offsets: Dict[Tuple[int, int], Tuple[int, TapSpec]] = {}
        external: Dict[Tuple[int, int], torch.Tensor] = {}
        total = 0
        if layout is not None:
            offsets, total = layout[2], layout[3]
        for n, s in (specs.items() if layout is None else ()):
            if s.slot < 0:
                continue
            key = (s.slot, s.layer)
            dst = tap_dst.get(n) if tap_dst else None
            if (dst is not None and key not in offsets and key not in external and dst.device == self.device and dst.dtype == s.dtype
                    and tuple(dst.shape) == tuple(s.shape) and dst.is_contiguous() and dst.data_ptr() % _ALIGN == 0
                    and cache_device is None and not remove_batch_dim):
                external[key] = dst
                continue
            if key in external:
                continue
            if key not in offsets:
                nbytes = _ESIZE[s.dtype]
                for dim in s.shape:
                    nbytes *= dim
                offsets[key] = (total, s)
                total += (nbytes + _ALIGN - 1) // _ALIGN * _ALIGN
        out_shape = head_out_shape(cfg, B)
        if layout is not None:
            out_off, total = layout[4], layout[5]
        else:
            out_off = total
            if run_head:
                nbytes = _ESIZE[cfg.dtype]
                for dim in out_shape:
                    nbytes *= dim
                total += (nbytes + _ALIGN - 1) // _ALIGN * _ALIGN
            if lkey is not None:
                if len(self._layouts) >= 16:
                    self._layouts.pop(next(iter(self._layouts)))
                    self._tap_arrays.clear()
                # (specs, out_name, offsets, tap bytes, out_off, slab bytes): everything about this call that does not depend on the slab
                self._layouts[lkey] = (specs, out_name, offsets, out_off, out_off, total)
        slab = self.arena.acquire(total)
        base = slab.data_ptr()

        n_taps = len(offsets) + len(external)
        taps = self._tap_arrays.get((lkey, base)) if lkey is not None else None
        if taps is None:
            taps = (N.Tap * max(n_taps, 1))()
            for i, ((slot, layer), (off, _)) in enumerate(offsets.items()):
                taps[i] = N.Tap(slot=slot, layer=layer, dst=base + off)
            for i, ((slot, layer), dst) in enumerate(external.items()):
                taps[len(offsets) + i] = N.Tap(slot=slot, layer=layer, dst=dst.data_ptr())
            if lkey is not None:
                if len(self._tap_arrays) >= 64:
                    self._tap_arrays.clear()
                self._tap_arrays[(lkey, base)] = taps
        ws = self._get_workspace(B)
        cur = torch.cuda.current_stream(self.device)
        stream = cur.cuda_stream
        # one plan = one workspace: a call on another stream than the previous one (the store's harvest prefetch runs on a
        # side stream, sae/store.py) waits for that one to finish with it
        last = getattr(self, "_last_use", None)
        if last is not None and last[0] != stream:
            cur.wait_event(last[1])
        if resid_in is None and not exit_stage:
            self._launch_full(images, B, n_blocks, run_head, taps, n_taps, ws, (base + out_off) if run_head else None, stream)
        else:
            ap = [a.data_ptr() for a in acts] + [None] * (3 - len(acts))
            N.check(self.lib.pv_vit_forward_stage(self._plan, images.data_ptr() if resid_in is None else None,
                                                  None if resid_in is None else resid_in.data_ptr(), ap[0], ap[1], ap[2], B,
                                                  first_block, entry_stage, n_blocks, exit_stage, int(run_head), taps,
                                                  n_taps, ws.data_ptr(), ws.numel(),
                                                  (base + out_off) if run_head else None, stream),
                    "pv_vit_forward_stage")
        self.n_forward += 1
        ev = last[1] if last is not None else torch.cuda.Event()
        ev.record(cur)
        self._last_use = (stream, ev)

        typed: Dict[Tuple[int, torch.dtype], torch.Tensor] = {}

        def view(src: torch.Tensor, off: int, s_dtype: torch.dtype, shape: Tuple[int, ...]) -> torch.Tensor:
            # ONE tensor op per entry: a strided window into the slab seen as s_dtype (214 entries per all-hooks call)
            base_t = typed.get((id(src), s_dtype))
            if base_t is None:
                base_t = typed[(id(src), s_dtype)] = src.view(s_dtype)
            return base_t.as_strided(shape, _contiguous_strides(shape), off // _ESIZE[s_dtype])

        to_cpu = cache_device is not None and torch.device(cache_device).type == "cpu"
        src = self.mirror.copy_from(slab, total) if (to_cpu and names) else slab
        cache: Dict[str, torch.Tensor] = {}
        for n in names:
            s = specs[n]
            if s.slot < 0:
                t = self._pos_embed_view(model, B)
                if cache_device is not None:
                    t = t.to(cache_device)
            elif (s.slot, s.layer) in external:
                t = external[(s.slot, s.layer)]
            else:
                off, _ = offsets[(s.slot, s.layer)]
                t = view(src, off, s.dtype, s.shape)
                if cache_device is not None and not to_cpu:
                    t = t.to(cache_device)
            cache[n] = t[0] if remove_batch_dim else t
        if run_head:
            out = view(slab, out_off, cfg.dtype, out_shape)
        elif (specs[out_name].slot, specs[out_name].layer) in external:
            out = external[(specs[out_name].slot, specs[out_name].layer)]
        else:
            off, s = offsets[(specs[out_name].slot, specs[out_name].layer)]
            out = view(slab, off, s.dtype, s.shape)
        return out, cache


class NativeText(NativeViT):
    """Owns one text plan (pv_text_plan_create) for one (config, dtype, device): HookedTextTransformer's forward on the same
    blocks, arena, weight-change detection and workspace cache as NativeViT; only the plan's ends differ."""

    def __init__(self, cfg, device: torch.device, causal: bool = True):
        self.causal = bool(causal)
        super().__init__(cfg, cfg.context_length, device)

    def _create_plan(self) -> None:
        cfg = self.cfg
        desc = N.TextDesc(
            n_layers=cfg.n_layers, d_model=cfg.d_model, n_heads=cfg.n_heads, d_head=cfg.d_head, d_mlp=cfg.d_mlp,
            context_length=cfg.context_length, vocab_size=cfg.vocab_size, n_classes=cfg.n_classes,
            has_head=int(cfg.return_type != "pre_logits"), normalize_output=int(bool(cfg.normalize_output)),
            causal=int(self.causal), activation=N.PV_ACT[cfg.activation_name],
            dtype=N.PV_DTYPE_BF16 if cfg.dtype == torch.bfloat16 else N.PV_DTYPE_F32, eps=float(cfg.eps),
            attn_scale=float(cfg.d_head ** 0.5) if cfg.use_attn_scale else 1.0)
        N.check(self.lib.pv_text_plan_create(C.byref(desc), C.byref(self._plan)), "pv_text_plan_create")

    @staticmethod
    def supported(cfg) -> Optional[str]:
        """None if a text plan can be built for this config, else why not (the shape rules themselves are the plan's: its own
        error text is passed through by the caller)."""
        if cfg.dtype not in (torch.float32, torch.bfloat16):
            return f"dtype {cfg.dtype}"
        if cfg.normalization_type != "LN":
            return f"normalization_type {cfg.normalization_type}"
        if cfg.activation_name not in N.PV_ACT:
            return f"activation {cfg.activation_name}"
        if cfg.attn_only or cfg.use_bert_block:
            return "architecture variant"
        return None

    def _collect(self, model) -> Tuple[N.TextWeights, list]:
        keep: List[torch.Tensor] = []
        P = self._borrow(keep)
        L = self._collect_layers(model, P)
        has_head = self.cfg.return_type != "pre_logits"
        W = N.TextWeights(
            token_embed=P(model.token_embed.weight), pos_embed=P(model.pos_embed),
            ln_final_w=P(model.ln_final.w), ln_final_b=P(model.ln_final.b),
            W_H=P(model.head.W_H) if has_head else None, b_H=P(model.head.b_H) if has_head else None,
            layers=C.cast(L, C.POINTER(N.VitLayerWeights)))
        return W, [keep, L]

    def _plan_slots(self, model) -> list:
        slots = self._block_slots(model)
        slots += [(model.token_embed, "weight"), (model, "pos_embed"), (model.ln_final, "w"), (model.ln_final, "b")]
        if self.cfg.return_type != "pre_logits":
            slots += [(model.head, "W_H"), (model.head, "b_H")]
        return slots

    def _set_weights(self, W, nbytes: int, stream: int) -> None:
        N.check(self.lib.pv_text_plan_set_weights(self._plan, C.byref(W), self._shadow.data_ptr(), nbytes, stream),
                "pv_text_plan_set_weights")

    def _check_input(self, tokens: torch.Tensor) -> torch.Tensor:
        if tokens.ndim != 2 or tokens.shape[1] != self.cfg.context_length:
            raise ValueError(f"expected tokens [B,{self.cfg.context_length}], got {tuple(tokens.shape)}")
        return tokens.to(torch.int64).contiguous()          # (int32 ids are widened on the device)

    def _launch_full(self, inp, B, n_blocks, run_head, taps, n_taps, ws, out_ptr, stream) -> None:
        if n_blocks != self.cfg.n_layers:
            raise N.NativeError("the text plan runs all blocks")
        N.check(self.lib.pv_text_forward(self._plan, inp.data_ptr(), B, int(run_head), taps, n_taps, ws.data_ptr(), ws.numel(),
                                         out_ptr, stream),
                "pv_text_forward")

    def _pos_embed_view(self, model, B: int) -> torch.Tensor:
        """hook_pos_embed: the parameter slice [T, d], no batch dimension (base_text_transformer.py:139)"""
        return model.pos_embed.detach()[: self.cfg.context_length]
