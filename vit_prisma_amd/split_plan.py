"""The split native plan: ``HookedViT.run_with_cache`` / ``run_with_hooks`` stay on the HIP plan while forward hooks (or modules
spliced in place of HookPoints, HookedSAEViT) sit inside the blocks.  The plan is split at each hooked point, the hooks run between
the segments as Python callbacks, the next segment resumes from what they return (pv_vit_forward_stage).  Hooks on the embedding /
final stage run that stage on the model's own modules; a block whose forward a hook changes in a way no plan segment computes runs
on its module (or only its head does, hooks on its per-head inputs), the blocks around it stay on the plan.

The block's structure is written down once: BLOCK (one row per HookPoint, in firing order: transformer_block.py:80-138,
attention.py:126-184, mlp.py:65-80) and EXIT (what a segment that stops at each PV_STAGE_* position hands on).  Everything below,
and the block part of tap_plan.hook_order, is read from these two tables."""
from __future__ import annotations

import re
from contextlib import contextmanager
from dataclasses import dataclass, field
from typing import Callable, Dict, Optional, Set, Tuple

import torch
import torch.nn.functional as F

from .hooked_root_module import names_filter_to_fn
from .tap_plan import resolve_n_blocks

# positions inside a block where the plan can be split (PV_STAGE_*, include/pv_native.h); position NPOS * l + s is stage s of
# block l, NPOS * (l + 1) the block's end (= the next block's ENTRY).  Stage s computes what lies between positions s and s + 1.
ENTRY, LN1, QKV, SCORES, PATTERN, Z, MID, LN2, MLP_PRE, MLP_POST = range(10)
NPOS = 10


@dataclass(frozen=True)
class Row:
    sub: str            # the HookPoint's name inside blocks.<l>.
    kind: str           # the key of a hook served at `pos`
    pos: int            # where it fires: the position whose hooks see it
    flag: str = ""      # the config flag that makes the point fire (flag-gated points)
    src: str = ""       # flag-gated: the tapped point its value is derived from ...
    how: str = ""       # ... and how: "heads" a per-head view (hooked: the block's head runs on module code), "result" z against
                        # W_O per head (attention.py:155-183), "copy" its own copy (transformer_block.py:125-129)


BLOCK = (
    Row("hook_resid_pre", "pre", ENTRY),
    Row("hook_attn_in", "attn_in", ENTRY, "use_attn_in", "hook_resid_pre", "heads"),
    Row("hook_q_input", "q_input", ENTRY, "use_split_qkv_input", "hook_resid_pre", "heads"),
    Row("hook_k_input", "k_input", ENTRY, "use_split_qkv_input", "hook_resid_pre", "heads"),
    Row("hook_v_input", "v_input", ENTRY, "use_split_qkv_input", "hook_resid_pre", "heads"),
    Row("ln1.hook_scale", "ln1s", LN1),
    Row("ln1.hook_normalized", "ln1n", LN1),
    Row("attn.hook_q", "q", QKV),
    Row("attn.hook_k", "k", QKV),
    Row("attn.hook_v", "v", QKV),
    Row("attn.hook_attn_scores", "scores", SCORES),
    Row("attn.hook_pattern", "pattern", PATTERN),
    Row("attn.hook_z", "z", Z),
    Row("attn.hook_result", "result", MID, "use_attn_result", "attn.hook_z", "result"),
    Row("hook_attn_out", "attn", MID),
    Row("hook_resid_mid", "mid", MID),
    Row("hook_mlp_in", "mlpin", LN2, "use_hook_mlp_in", "hook_resid_mid", "copy"),
    Row("ln2.hook_scale", "ln2s", LN2),
    Row("ln2.hook_normalized", "ln2n", LN2),
    Row("mlp.hook_pre", "mlppre", MLP_PRE),
    Row("mlp.hook_post", "mlppost", MLP_POST),
    Row("hook_mlp_out", "mlp", NPOS),
    Row("hook_resid_post", "post", NPOS),
)


@dataclass(frozen=True)
class Exit:
    taps: Tuple[str, ...]        # kinds a segment stopping here must tap: what the hooks here see (residual positions: the sum first)
    carried: str                 # the residual stream the rest of the block adds to (tapped when the segment computes it)
    acts: Tuple[str, ...] = ()   # kinds handed to the next segment (act_in), after the hooks
    delta: str = ""              # residual positions: the summand a hook there rebuilds the sum from
    ln: str = ""                 # LayerNorm positions: the module


EXIT = {
    ENTRY: Exit(("post",), "mid", delta="mlp"),             # the previous block's end; then this block's hook_resid_pre fires
    LN1: Exit(("ln1s", "ln1n"), "pre", ("ln1n",), ln="ln1"),
    QKV: Exit(("q", "k", "v"), "pre", ("q", "k", "v")),
    SCORES: Exit(("scores",), "pre", ("scores", "v")),      # (the resumed attention core reads v next to the edited scores / pattern)
    PATTERN: Exit(("pattern",), "pre", ("pattern", "v")),
    Z: Exit(("z",), "pre", ("z",)),
    MID: Exit(("mid",), "pre", delta="attn"),
    LN2: Exit(("ln2s", "ln2n"), "mid", ("ln2n",), ln="ln2"),
    MLP_PRE: Exit(("mlppre",), "mid", ("mlppre",)),
    MLP_POST: Exit(("mlppost",), "mid", ("mlppost",)),
}

ROW = {r.sub: r for r in BLOCK}
KIND = {r.kind: r for r in BLOCK}
EMBED_NAMES = ("hook_embed", "hook_pos_embed", "hook_full_embed", "ln_pre.hook_scale", "ln_pre.hook_normalized", "hook_ln_pre")
FINAL_NAMES = ("ln_final.hook_scale", "ln_final.hook_normalized", "hook_ln_final", "hook_post_head_pre_normalize")
_BLOCK = re.compile(r"blocks\.(\d+)\.(.+)")


def _row(name: str):
    """(block index, Row) of a block's HookPoint; (None, None) elsewhere"""
    m = _BLOCK.fullmatch(name)
    return (int(m.group(1)), ROW.get(m.group(2))) if m else (None, None)


@dataclass
class HookSites:
    """Where the registered forward hooks (and spliced modules) sit, as the split plan serves them."""
    at: Dict[int, Dict[str, Callable]] = field(default_factory=dict)     # in-block: {position: {kind: hook}}
    embed: Dict[str, Callable] = field(default_factory=dict)             # embedding stage (block 0's hook_resid_pre included)
    final: Dict[str, Callable] = field(default_factory=dict)             # final stage
    module_blocks: Set[int] = field(default_factory=set)                 # blocks that run on their own module
    head_blocks: Set[int] = field(default_factory=set)                   # blocks that run their head (up to q, k, v) on module code


def hook_sites(model) -> Optional[HookSites]:
    """The forward hooks of `model` by where they sit, or None when some hook (a backward hook, a forward hook on a point the plan
    cannot be split at, a spliced module in another dtype or elsewhere) cannot be served."""
    cfg, out = model.cfg, HookSites()
    spliced = model._spliced()
    for name, mod in spliced.items():
        # a module spliced in place of a HookPoint is called on the tapped tensor like that point's hooks would be.  On a LayerNorm
        # point, on block 0's entry or on the source of an enabled flag-gated point (which then sees the module's output, no tap)
        # its block runs on its module
        if getattr(mod, "dtype", cfg.dtype) != cfg.dtype:
            return None
        l, row = _row(name)
        if row is None or row.flag:                      # (on the embedding / final stage: what that stage's module code calls)
            stage = out.embed if name in EMBED_NAMES else out.final if name in FINAL_NAMES else None
            if stage is None:
                return None
            stage[name] = mod
            continue
        if (row.pos == ENTRY and l == 0) or row.sub.startswith("ln") or any(r.src == row.sub and getattr(cfg, r.flag) for r in BLOCK):
            out.module_blocks.add(l)
        else:
            out.at.setdefault(NPOS * l + row.pos, {})[row.kind] = mod
    for name, hp in model.hook_dict.items():
        if hp._backward_hooks:
            return None
        if not hp._forward_hooks or (spliced and any(name.startswith(s + ".") for s in spliced)):
            continue                                     # (a spliced module's own HookPoints fire inside its forward)
        if name in EMBED_NAMES or name == "blocks.0.hook_resid_pre":
            out.embed[name] = hp
            continue
        if name in FINAL_NAMES:
            out.final[name] = hp
            continue
        l, row = _row(name)
        if row is None:
            return None
        if row.flag and not getattr(cfg, row.flag):
            continue                                     # (never called with its flag off: the hook cannot fire)
        if row.sub.startswith("ln") and cfg.normalization_type not in ("LN", "LNPre"):
            return None
        if row.how == "heads" or (row.sub.startswith("ln1.") and (cfg.use_attn_in or cfg.use_split_qkv_input)):
            out.head_blocks.add(l)                       # (ln1's points carry a head dimension there)
        else:
            out.at.setdefault(NPOS * l + row.pos, {})[row.kind] = hp
    return out


@contextmanager
def recording(model, names, rec: Dict[str, torch.Tensor]):
    """Notes what the HookPoints of `names` pass on while module code runs: a hook behind the caller's own, so the value is the
    post-hook one, as in the cache of the PyTorch path."""
    added = []
    for n in names:
        hp = model.hook_dict.get(n)
        if hp is not None:
            hp.add_hook(lambda t, hook, n=n: rec.__setitem__(n, t))
            added.append((hp, hp.fwd_hooks[-1]))
    try:
        yield rec
    finally:
        for hp, h in added:
            h.hook.remove()
            hp.fwd_hooks.remove(h)


def run(model, x: torch.Tensor, names_filter=None, device=None, remove_batch_dim: bool = False, stop_at_layer: Optional[int] = None,
        **_ignored):
    """The caching run on the HIP plan: (output, {name: tensor} in firing order)."""
    from .tap_plan import hook_order
    cfg = model.cfg
    sites = hook_sites(model) or HookSites()
    keep = names_filter_to_fn(names_filter)
    run_head = stop_at_layer is None
    n_blocks = cfg.n_layers if run_head else resolve_n_blocks(cfg.n_layers, stop_at_layer)
    order = hook_order(cfg, n_blocks, run_head)
    spliced = model._spliced()
    if spliced:                                          # a splice's own HookPoints stand where the replaced point stood
        order = [k for n in order for k in ([k for k in model.hook_dict if k.startswith(n + ".")] if n in spliced else [n])]
    wanted = [n for n in order if keep(n)]
    # what lies behind stop_at_layer never fires (a hook at the very end only if its point is produced)
    end = NPOS * n_blocks
    at = {q: k for q, k in sites.at.items() if q < end or (q == end and any(KIND[x].pos == NPOS for x in k))}
    final = sites.final if run_head else {}
    module = {l for l in sites.module_blocks if l < n_blocks}
    head = {l for l in sites.head_blocks if l < n_blocks} - sites.module_blocks
    flags = any(getattr(cfg, r.flag) for r in BLOCK if r.flag)
    nv = model._get_native(x.device)
    if not (spliced or flags or at or sites.embed or final or module or head):
        tap_dst = getattr(model, "_tap_dst", None)      # (the activation store's own buffer slice, sae/store.py)
        return nv.forward(model, x, wanted, n_blocks, run_head, cache_device=device, remove_batch_dim=remove_batch_dim,
                          **({"tap_dst": tap_dst} if tap_dst else {}))
    # the splices' HookPoints are recorded while they run; a flag-gated point is recorded where module code fires it or where its hook
    # is served, and otherwise derived from the tap it comes from
    inner = [n for n in wanted if any(n.startswith(s + ".") for s in spliced)]
    need = set(wanted) - set(inner)
    for n in wanted:
        l, row = _row(n)
        if row is not None and row.flag:
            need.add(f"blocks.{l}.{row.src}")
    names = [n for n in order if n in need]
    got: Dict[str, torch.Tensor] = {}
    with recording(model, inner, got):
        out = _Run(model, nv, x, names, got).stages(n_blocks, run_head, at, sites.embed, final, sorted(module | head), head)
    headed = cfg.use_attn_in or cfg.use_split_qkv_input
    cache: Dict[str, torch.Tensor] = {}
    for n in wanted:
        t = got.get(n)
        if t is None:
            l, row = _row(n)
            src = got.get(f"blocks.{l}.{row.src}") if row is not None and row.flag else None
            if src is None:
                continue                                 # (behind stop_at_layer, or a spliced module that never ran)
            if row.how == "result":
                t = torch.einsum("bphd,hdm->bphm", src, model.blocks[l].attn.W_O)
            elif row.how == "copy":
                t = src.clone()                          # (its own storage, like the reference's)
            else:
                t = src.unsqueeze(2).expand(-1, -1, cfg.n_heads, -1)
        elif headed and n.endswith(("ln1.hook_scale", "ln1.hook_normalized")) and t.ndim == 3:
            t = t.unsqueeze(2).expand(-1, -1, cfg.n_heads, -1)
        # (the head-dimension entries are stride-0 views: an in-place write into one raises instead of reaching its siblings)
        if device is not None:
            t = t.to(device)
        cache[n] = t[0] if remove_batch_dim else t
    return out, cache


def _layer_norm(mod, x: torch.Tensor, scale: Optional[torch.Tensor] = None):
    """(hook_scale, hook_normalized) of LayerNorm `mod` on x as the module computes them (layer_norm.py:38-45, 84-93), given the
    scale when it was edited"""
    if mod.cfg.dtype not in (torch.float32, torch.float64):
        x = x.to(torch.float32)
    x = x - x.mean(-1, keepdim=True)
    if scale is None:
        scale = (x.pow(2).mean(-1, keepdim=True) + mod.eps).sqrt()
    out = x / scale
    return scale, (out * mod.w + mod.b if hasattr(mod, "w") else out)


class _Run:
    """One split run: `names` the requested points in firing order, `got` what it caches."""

    def __init__(self, model, nv, x, names, got):
        self.model, self.nv, self.x, self.names, self.got = model, nv, x, names, got
        self.wanted = set(names)
        self.span = {n: _span(n, model.cfg.n_layers) for n in names}
        self.taps = [n for n in names if not getattr(_row(n)[1], "flag", "")]      # (flag-gated points are no taps of the plan)
        tap_dst = getattr(model, "_tap_dst", None)        # (the activation store's own buffer slice, sae/store.py)
        self.tap_dst = {"tap_dst": tap_dst} if tap_dst else {}

    def keep(self, kind: str, l: int, t: torch.Tensor) -> None:
        n = f"blocks.{l}.{KIND[kind].sub}"
        if n in self.wanted:
            self.got[n] = t

    def record(self, names):
        return recording(self.model, [n for n in names if n in self.wanted], self.got)

    def stages(self, n_blocks, run_head, at, embed, final, tblocks, hblocks):
        """Embedding stage -> blocks 0 .. n_blocks - 1 -> final stage, where the blocks of `tblocks` run on module code (those of
        `hblocks` only up to q, k, v) and the runs of blocks between them on the HIP plan, resumed from / stopped at the residual
        stream (or entered at PV_STAGE_QKV behind a head on module code)."""
        model, cfg = self.model, self.model.cfg
        resid, b, entry, acts = None, 0, ENTRY, ()    # the next plan run enters block b at `entry` with these activations
        if embed:
            # base_vit.py:169-185 on the model's own modules (block 0's hook_resid_pre fires here unless block 0 runs on its module)
            with_pre = n_blocks > 0 and not (tblocks and tblocks[0] == 0)
            with self.record(EMBED_NAMES + (("blocks.0.hook_resid_pre",) if with_pre else ())):
                x = self.x.to(cfg.dtype)
                e = model.hook_embed(model.embed(x))
                if cfg.use_cls_token:
                    e = torch.cat((model.cls_token.expand(x.shape[0], -1, -1), e), dim=1)
                resid = e + model.hook_pos_embed(model.pos_embed(x))
                model.hook_full_embed(resid)                         # observe-only
                if cfg.layer_norm_pre:
                    resid = model.hook_ln_pre(model.ln_pre(resid))
                if with_pre:
                    resid = model.blocks[0].hook_resid_pre(resid)
            resid = resid.contiguous()
        head_on_plan = run_head and not final
        for L in tblocks + [None]:
            stop = n_blocks if L is None else L
            head_here = L is None and head_on_plan
            if stop > b or head_here or resid is None:
                # this run's hooks: strictly inside it, at its end only what belongs to its last block (the next block's
                # hook_resid_pre fires inside that block's module); at its start block b's hook_resid_pre by hand
                sub = {q: k for q, k in at.items() if NPOS * b + entry < q < NPOS * stop}
                if stop > b and NPOS * stop in at:
                    k = at[NPOS * stop] if L is None else {k: v for k, v in at[NPOS * stop].items() if KIND[k].pos == NPOS}
                    if k:
                        sub[NPOS * stop] = k
                if resid is not None and b > 0 and stop > b and entry == ENTRY:
                    pre = at.get(NPOS * b, {}).get("pre")
                    if pre is not None:
                        resid = pre(resid)
                    self.keep("pre", b, resid)
                resid = self.segments(resid, b, entry, acts, stop, head_here, sub)
                entry, acts = ENTRY, ()
            if L is None:
                break
            if L in hblocks:
                resid, acts = self.head_on_module(L, resid)
                b, entry = L, QKV
                continue
            resid, rec = model._torch_block_stage(L, resid, self.wanted)
            self.got.update(rec)
            b = L + 1
        if final:
            # base_vit.py:192-217 on the model's own modules
            with self.record(FINAL_NAMES):
                x = model.ln_final(resid)
                model.hook_ln_final(x)                               # observe-only
                if cfg.classification_type == "gaap":
                    x = x.mean(dim=1)
                elif cfg.classification_type == "cls":
                    cls_tok = x[:, 0]
                    if "dino-vitb" in cfg.model_name:
                        x = torch.cat((cls_tok.unsqueeze(-1), x[:, 1:].mean(dim=1).unsqueeze(-1)), dim=-1)
                    else:
                        x = cls_tok
                if cfg.return_type != "pre_logits":
                    x = model.head(x)
                model.hook_post_head_pre_normalize(x)                # observe-only
                resid = F.normalize(x, dim=-1) if cfg.normalize_output else x
        return resid

    def head_on_module(self, l: int, resid: torch.Tensor):
        """Block l up to its q, k, v on the module's own code (transformer_block.py:80-109, attention.py:186-244), where the HookPoints
        of the per-head inputs live: (resid_pre, (q, k, v)); the plan resumes at PV_STAGE_QKV."""
        cfg, blk = self.model.cfg, self.model.blocks[l]
        with self.record(f"blocks.{l}.{r.sub}" for r in BLOCK if r.pos <= QKV):
            resid_pre = blk.hook_resid_pre(resid)
            attn_in = resid_pre
            if cfg.use_attn_in or cfg.use_split_qkv_input:
                attn_in = resid_pre.unsqueeze(2).expand(-1, -1, cfg.n_heads, -1)
            if cfg.use_attn_in:
                attn_in = blk.hook_attn_in(attn_in.clone())
            if cfg.use_split_qkv_input:
                q_in, k_in, v_in = blk.hook_q_input(attn_in.clone()), blk.hook_k_input(attn_in.clone()), blk.hook_v_input(attn_in.clone())
            else:
                q_in = k_in = v_in = attn_in
            q, k, v = blk.attn.calculate_qkv_matrices(blk.ln1(q_in), blk.ln1(k_in), blk.ln1(v_in))
        return resid_pre.contiguous(), (q.contiguous(), k.contiguous(), v.contiguous())

    def segments(self, resid, b: int, entry: int, acts, stop: int, run_head: bool, at) -> torch.Tensor:
        """Blocks b .. stop - 1 (+ the head) on the HIP plan, from the pixels (resid None) or resumed at position `entry` of block b
        from `resid` and `acts`, split at the positions of `at`: [p0, q1) -> hooks at q1 -> [q1, q2) -> ... -> [qk, end)."""
        model, nv, got, span, L = self.model, self.nv, self.got, self.span, self.model.cfg.n_layers
        end = NPOS * stop
        p0, out, from_px = NPOS * b + entry, None, resid is None
        for q in sorted(at) + [None]:
            last = q is None
            p1 = end if last else q
            b1, s1 = divmod(p1, NPOS)
            first_px = from_px and p0 == 0
            made = lambda n: first_px or (span[n] if n in span else _span(n, L))[0] >= p0      # noqa: E731  (computed in this segment)
            bound = NPOS * L + 1 if last and run_head else p1
            seg = [n for n in self.taps if made(n) and span[n][1] < bound]
            hooks = {} if last else at[q]
            ex, blk = EXIT[s1], (b1 if s1 else b1 - 1)
            nm = lambda kind, l=blk: f"blocks.{l}.{KIND[kind].sub}"  # noqa: E731
            rebuild = bool(ex.delta) and (ex.delta in hooks or any(KIND[k].flag for k in hooks))
            forced = []
            if not last:
                # the taps the hooks here see, and what the rest of the block needs that no later segment computes: the carried
                # stream, v for a resumed attention core, the source of a served flag-gated point -- where this segment computes it
                extra = [nm(k) for k in ex.acts if k not in ex.taps] + [f"blocks.{blk}.{KIND[k].src}" for k in hooks if KIND[k].flag]
                extra += [nm(ex.carried)] if rebuild or not ex.delta else []
                forced = [nm(k) for k in ex.taps + ((ex.delta,) if rebuild else ())] + [n for n in extra if made(n)]
            seg_in, c = resid, {}
            if p0 < p1 or (last and run_head) or first_px:
                req = seg + [n for n in dict.fromkeys(forced) if n not in seg]
                out, c = nv.forward(model, self.x if first_px else None, req, b1, last and run_head, first_block=p0 // NPOS,
                                    resid_in=None if first_px else resid, entry_stage=p0 % NPOS, exit_stage=s1, act_in=acts,
                                    **(self.tap_dst if first_px and last else {}))
                got.update((k, v) for k, v in c.items() if k in self.wanted)
            elif last:
                out = resid                                  # nothing left to run: the hooked residual is the output
            if last:
                break
            prev_acts, acts = acts, ()
            resid = c.get(nm(ex.carried), seg_in)              # the residual stream the rest of the block adds to
            if ex.delta:
                # the sum as the plan computed it -- rebuilt with the kernel's rounding when a hook edits the summand
                # (transformer_block.py:117-124, 131-134) -- then the sum's hooks
                total = c[nm(ex.taps[0])]
                if rebuild:
                    d = c[nm(ex.delta)]
                    if "result" in hooks:
                        # use_attn_result: z against W_O per head, the hook on the per-head results, their sum + b_O is what the
                        # block adds (attention.py:155-183)
                        attn = model.blocks[blk].attn
                        z = c[nm("z")] if nm("z") in c else prev_acts[0]
                        r = hooks["result"](torch.einsum("bqhe,hed->bqhd", z, attn.W_O))
                        self.keep("result", blk, r)
                        d = r.sum(dim=2) + attn.b_O
                    if ex.delta in hooks:
                        d = hooks[ex.delta](d)
                    self.keep(ex.delta, blk, d)
                    total = resid + d.to(resid.dtype)
                if ex.taps[0] in hooks:
                    total = hooks[ex.taps[0]](total)
                self.keep(ex.taps[0], blk, total)
                resid = total
                if s1 == ENTRY and p1 < end:
                    if "pre" in hooks:
                        resid = hooks["pre"](resid)
                    self.keep("pre", b1, resid)
            elif ex.ln:
                # hook_scale, hook_normalized recomputed from the (edited) scale as the module does, then hook_normalized's own
                # hooks; the block resumes from the fp32 tensor they leave.  The LayerNorm's input is the carried stream -- or what
                # a flag-gated point between them returns (hook_mlp_in: its hook sees a copy of resid_mid)
                mod = getattr(model.blocks[b1], ex.ln)
                s_k, n_k = ex.taps
                ln_in, scale, norm = resid, c[nm(s_k)], c[nm(n_k)]
                for r in BLOCK:
                    if r.pos == s1 and r.flag and r.kind in hooks:
                        ln_in = hooks[r.kind](ln_in.clone())
                        self.keep(r.kind, b1, ln_in)
                        scale, norm = _layer_norm(mod, ln_in)
                if s_k in hooks:
                    scale = hooks[s_k](scale)
                    norm = _layer_norm(mod, ln_in, scale)[1]
                if n_k in hooks:
                    norm = hooks[n_k](norm)
                self.keep(s_k, b1, scale)
                self.keep(n_k, b1, norm)
                acts = (norm,)
            else:
                # inside the attention half / the MLP: the hooks see the stage's activations, the block resumes from what they return
                vals = {}
                for k in ex.taps:
                    t = c[nm(k)]
                    if k in hooks:
                        t = hooks[k](t)
                    self.keep(k, b1, t)
                    vals[k] = t
                acts = tuple(vals[k] if k in vals else c[nm(k)] if nm(k) in c else prev_acts[-1] for k in ex.acts)
            p0 = p1
        return resid if out is None else out


def _span(name: str, n_layers: int) -> Tuple[int, int]:
    """(the stage that produces a point, the stage a segment must reach to tap it): they differ for hook_resid_pre, produced by the
    previous block's last stage but handed on by hand where the plan is split at the block's entry.  -1: the embedding stage,
    NPOS * n_layers: the final stage."""
    l, row = _row(name)
    if row is None:
        st = -1 if name in EMBED_NAMES else NPOS * n_layers
        return st, st
    p = NPOS * l + row.pos
    return p - 1, max(p - 1, NPOS * l)
