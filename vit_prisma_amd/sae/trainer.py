"""VisionSAETrainer: the SAE training loop behind the reference's trainer API.

Same constructor / ``train_step`` / ``run`` contract as
/root/reference/src/vit_prisma/sae/train_sae.py:61-861 (signature ``(cfg, model, dataset,
eval_dataset=None)``, ``train_step`` argument names and 7-tuple, ``run() -> sae``).  The order of
operations inside a step is the reference's (:278-411): renorm decoder -> zero_grad -> forward ->
firing statistics -> backward -> clip_grad_norm_ -> remove parallel gradient -> Adam -> scheduler.

On an MI355X the step runs on ``NativeSAE`` (HIP kernels) directly on the module's parameter storage; Adam moments
live in the engine.  ``train_step`` resolves the route once (``_native_kind``: "topk" / "relu" / "gated", under the
conditions listed in ``_native_limits``) and ``_native_step`` takes it: ``_step_topk`` (the k-sparse step, also a
top-k Transcoder, ghost gradients included), ``_step_dense`` (ReLU + L1 and the gated SAE), ``_step_feature_parallel``.
Everything else (other activations, widths beyond the limits, CPU) takes the PyTorch path below, which is the
reference algorithm verbatim; on a GPU the trainer says once which condition sent it there (``_native_why_not``).

Data parallel (new functionality, SURVEY.md section 8e -- the reference is single-process): one process
per GPU, each with its share of the global token batch and a 1/W shard of the OPTIMIZER, by feature
(rows j in [r d_sae/W, (r+1) d_sae/W) of W_enc^T, W_dec, b_enc -- contiguous slices of the flat buffers):

    all-reduce     768 floats            global batch mean for the loss normaliser (sae.py:145), before the forward
    reduce-scatter gW_enc^T, gW_dec, gb_enc   every rank receives the summed gradient rows of ITS features
    all-reduce     gb_dec | fire counts | loss, mse, l0     one small bucket (768 + d_sae + 3 floats)
    all-reduce     1 float               sum of the ranks' squared-norm terms: the clip norm is the GLOBAL gradient
                                         norm exactly as in a single process (train_sae.py:394-397)
    (local)        clip -> project -> Adam on the rank's rows only: the 1.06 GB / step optimizer pass shrinks by W
    all-gather     W_enc^T, W_dec, b_enc rows    asynchronous: they ride RCCL's stream while this rank already harvests
                                         the next batch; waited for at the start of the next step

b_dec (768 floats) is updated redundantly and identically on every rank.  When d_sae is not divisible by 4 W the
trainer falls back to one all-reduce of the flat gradient buffer and a replicated optimizer.
"""
from __future__ import annotations

import os
from typing import Any, List, Optional

import torch
from torch.optim import Adam

from .config import VisionModelSAERunnerConfig
from .get_scheduler import get_scheduler
from .sae import StandardSparseAutoencoder
from .store import VisionActivationsStore, _dist_info


def _wandb():
    try:
        import wandb  # type: ignore
        return wandb
    except Exception:
        return None


# The numeric limits of the fused HIP steps and the sentences that state them (VisionSAETrainer._native_limits): every width a
# multiple of _MULT, of _MULT_DENSE on the dense GEMMs and in the ghost term; the {}-fields are filled by _native_why_not.
_MULT, _MULT_DENSE, _MAX_D_IN, _MAX_D_SAE, _MAX_K = 4, 8, 1280, 65536, 256
_D_IN = f"d_in = {{cfg.d_in}} (supported: multiples of {_MULT} up to {_MAX_D_IN} = ViT-H/14)"
_D_SAE = f"d_sae = {{cfg.d_sae}} (supported: multiples of {_MULT} up to {_MAX_D_SAE})"
_K = f"k = {{k}} (supported: 1..{_MAX_K})"
_TC_WIDTHS = (f"a transcoder with d_out != d_in and the skip connection / widths that are not multiples of {_MULT_DENSE} / "
              f"d_out > {_MAX_D_IN}")
_DENSE_WIDTHS = f"d_in = {{cfg.d_in}}, d_sae = {{cfg.d_sae}} (the ReLU + L1 and the gated steps: multiples of {_MULT_DENSE})"
_GHOST_WIDTH = f"ghost gradients with d_in = {{cfg.d_in}} (supported: multiples of {_MULT_DENSE})"
_NOT_AN_SAE = "a {kind} (supported: StandardSparseAutoencoder, GatedSparseAutoencoder, a Transcoder under cfg.is_transcoder)"


class VisionSAETrainer:
    def __init__(self, cfg: VisionModelSAERunnerConfig, model, dataset, eval_dataset=None, sparse_coder=None,
                 activations_store=None):
        self.cfg = cfg
        self.is_transcoder = bool(getattr(cfg, "is_transcoder", False))
        self.model = model
        self.dataset = dataset
        self.eval_dataset = eval_dataset
        self.bad_run_check = cfg.min_l0 is not None and cfg.min_explained_variance is not None
        torch.manual_seed(cfg.seed)
        if sparse_coder is None:                          # train_sae.py:72-81
            if self.is_transcoder:
                from .variants import Transcoder
                sparse_coder = Transcoder(cfg)
            elif cfg.architecture == "gated":
                from .variants import GatedSparseAutoencoder
                sparse_coder = GatedSparseAutoencoder(cfg)
            elif cfg.architecture in ("standard", "vanilla"):
                sparse_coder = StandardSparseAutoencoder(cfg)
            else:
                raise ValueError(f"Loading of {cfg.architecture} not supported")
        self.sparse_coder = sparse_coder
        self.sae = self.sparse_coder                      # legacy alias
        self.activations_store = activations_store
        if self.activations_store is None and cfg.use_cached_activations and not self.is_transcoder:
            from .store import CacheVisionActivationStore
            self.activations_store = CacheVisionActivationStore(cfg, *_dist_info())     # train_sae.py:138-139
        if self.activations_store is None and dataset is not None:
            self.activations_store = VisionActivationsStore(cfg, model, dataset, eval_dataset=eval_dataset,
                                                            num_workers=0)
        self.checkpoint_thresholds = self.get_checkpoint_thresholds()
        self._engine = None
        self._native_pref: Optional[bool] = None            # None = auto, True = native or raise, False = PyTorch path
        self._pending = []                                  # in-flight parameter all-gathers of the sharded optimizer
        self._small = None
        self.rank, self.world = _dist_info()
        self._feature_parallel: Optional[bool] = None       # multi-rank native top-k step: None = auto (feature parallel when d_sae
                                                            # divides by the world size), True / False = forced
        self._force_dist = False                            # see _mr
        self._fp = None                                     # FeatureParallelSAE (this rank's shard engine + choreography)
        self._fp_dirty = False                              # the module's parameters lag behind the shards
        self._fp_drop = False                               # use_feature_parallel(drop_replicas=True)
        self._target = None                                 # transcoder: the target activation of the current step
        self._warned_torch_path = False

    @property
    def _mr(self) -> bool:
        """Do the steps take their multi-rank form (collectives, sharded optimizer / feature shards)?  With more than one rank,
        or when ``force_distributed_paths`` asked for it in a process group of ONE rank -- the same calls on the same backend
        (the in-place reduce_scatter_tensor / all_gather_into_tensor / packed buckets on RCCL), which is how a one-GPU box
        executes the code an 8-GPU job runs."""
        return self.world > 1 or self._force_dist

    def force_distributed_paths(self, flag: bool = True) -> "VisionSAETrainer":
        import torch.distributed as dist
        if flag and not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError("force_distributed_paths needs an initialised torch.distributed process group")
        self._force_dist = bool(flag)
        return self

    def use_native(self, flag: Optional[bool]) -> "VisionSAETrainer":
        """True: the fused HIP step or an error; False: always the PyTorch path; None (default): native when supported."""
        self._native_pref = flag
        return self

    def use_feature_parallel(self, flag: Optional[bool] = True, drop_replicas: bool = False) -> "VisionSAETrainer":
        """How multi-rank native top-k steps are sharded.  True: by FEATURE (sae/feature_parallel.py: every rank keeps
        d_sae / world features and their optimizer state for good, sees the whole token batch, and only token-sized
        collectives cross the links); False: by token, with the optimizer sharded by feature (reduce-scatter of the gradient
        rows, all-gather of the updated parameter rows: 302 MB per 4096-token step at 768 -> 24576); None (default): feature
        parallel whenever d_sae is divisible by the world size -- by the measured per-rank phase times it is the faster of
        the two at every world size for the reference's 4096-token batch.  In the feature-parallel mode
        the module's own parameters are refreshed only by ``sync_parameters()`` (``checkpoint`` and the end of ``run`` call
        it).  drop_replicas: while the shards train, the module's two matrices (W_enc, W_dec: 2 x d_in x d_sae floats that no
        kernel reads in this mode) are released on every rank -- ``sae.W_enc`` / ``sae.W_dec`` are EMPTY between
        ``sync_parameters()`` calls, which allocate and fill them again (and the next step releases them again).  New
        functionality (the reference is single-process)."""
        self._feature_parallel = None if flag is None else bool(flag)
        self._fp_drop = bool(drop_replicas)
        return self

    def _use_tp(self, sae) -> bool:
        if not self._mr or self._feature_parallel is False:
            return False
        if self._feature_parallel is None:
            # auto: only where the feature-parallel kernels can run (pv_sae_tp_merge ranks the candidates of at most 8 ranks,
            # a shard must hold at least k features and a whole number of 4-feature groups); anything else -- two nodes, small
            # or odd shards -- takes the token-sharded step, which has no such limits.  use_feature_parallel(True) keeps the
            # hard error.
            d_sae, k = int(sae.cfg.d_sae), int((sae.cfg.activation_fn_kwargs or {}).get("k", 1))
            shard = d_sae // self.world
            return d_sae % self.world == 0 and self.world <= 8 and shard >= k and shard % 4 == 0 and k <= 64      # (pv_sae_tp_merge ranks <= 8 x 64)
        return True

    # ---- bookkeeping ------------------------------------------------------------------------------
    def get_checkpoint_thresholds(self) -> List[int]:
        if self.cfg.n_checkpoints > 0:
            t = self.cfg.total_training_tokens
            return list(range(0, t, max(t // self.cfg.n_checkpoints, 1)))[1:]
        return []

    def initialize_training_variables(self):
        dev = self.cfg.device
        act_freq_scores = torch.zeros(int(self.cfg.d_sae), device=dev)
        n_forward_passes_since_fired = torch.zeros(int(self.cfg.d_sae), device=dev)
        n_frac_active_tokens = 0
        optimizer = Adam(self.sparse_coder.parameters(), lr=self.cfg.lr)
        scheduler = get_scheduler(self.cfg.lr_scheduler_name, optimizer=optimizer,
                                  warm_up_steps=self.cfg.lr_warm_up_steps,
                                  training_steps=self.cfg.total_training_steps, lr_end=self.cfg.lr / 10)
        return act_freq_scores, n_forward_passes_since_fired, n_frac_active_tokens, optimizer, scheduler

    def initialize_geometric_medians(self):
        cfg = self.sparse_coder.cfg
        layers = cfg.hook_point_layer if isinstance(cfg.hook_point_layer, list) else [cfg.hook_point_layer]
        lid = layers.index(cfg.hook_point_layer) if not isinstance(cfg.hook_point_layer, list) else 0
        medians = {}
        if cfg.b_dec_init_method == "geometric_median":
            from .geometric_median import compute_geometric_median
            acts = self.activations_store.storage_buffer.detach()[:, lid, :]
            medians[lid] = compute_geometric_median(acts, maxiter=200).median
            out_median = None
            if self.is_transcoder:
                acts_out = self.activations_store.storage_buffer_out.detach()[:, lid, :]
                out_median = compute_geometric_median(acts_out, maxiter=200).median
            if self.world > 1:
                # every rank harvested different images: rank 0's median is THE initial b_dec (replicas must start equal)
                import torch.distributed as dist
                med = medians[lid].to(cfg.device).contiguous()
                dist.broadcast(med, src=0)
                medians[lid] = med
                if out_median is not None:
                    out_median = out_median.to(cfg.device).contiguous()
                    dist.broadcast(out_median, src=0)
            self.sparse_coder.initialize_b_dec_with_precalculated(medians[lid], out_median)
        elif cfg.b_dec_init_method == "mean":
            acts = self.activations_store.storage_buffer.detach()[:, lid, :]
            if self.world > 1:
                import torch.distributed as dist
                m = acts.float().mean(dim=0)
                dist.all_reduce(m)
                self.sparse_coder.b_dec.data = (m / self.world).to(self.sparse_coder.dtype)
            else:
                self.sparse_coder.initialize_b_dec_with_mean(acts)
        self.sparse_coder.train()
        return medians

    # ---- native engine ----------------------------------------------------------------------------
    def _native_limits(self, sae, x: Optional[torch.Tensor] = None):
        """(kind, [(holds, text), ...]): the fused HIP step that would serve this SAE -- "topk" (k-sparse step, pv_sae_step; also the
        top-k Transcoder), "relu" (ReLU / tanh-relu + L1: pv_sae_relu_step, sparse where the batch allows it, pv_sae_dense_step with
        ghost gradients), "gated" (a GatedSparseAutoencoder: pv_sae_gated_step_sparse, or pv_sae_gated_topk_step for its top-k form), None
        for any other activation -- and EVERY condition it runs under, each with the sentence that tells the user about it (its {}-fields
        are filled by ``_native_why_not``).  The one statement of these limits: ``_native_kind`` takes the step when all hold,
        ``_native_why_not`` lists those that do not.  The last entry is the only one that needs the GPU."""
        from .variants import GatedSparseAutoencoder, Transcoder
        cfg = sae.cfg
        act, k, d_in, d_sae = cfg.activation_fn_str, cfg.activation_fn_kwargs.get("k", 0), int(cfg.d_in), int(cfg.d_sae)
        d_out = int(getattr(cfg, "d_out", d_in))
        gated, tc, ghost = isinstance(sae, GatedSparseAutoencoder), isinstance(sae, Transcoder), bool(cfg.use_ghost_grads)
        kind = None if act not in (("relu", "topk") if gated else ("topk", "relu", "tanh-relu")) else \
            "gated" if gated else "topk" if act == "topk" else "relu"
        return kind, [
            # a Transcoder runs on the same steps (pv_sae_transcoder) once train_step has split its target off the batch
            (isinstance(sae, StandardSparseAutoencoder) or gated or (tc and self._target is not None), _NOT_AN_SAE),
            (cfg.dtype == torch.float32, "dtype {cfg.dtype} (the fused steps keep fp32 master weights)"),
            (d_in <= _MAX_D_IN and d_in % _MULT == 0, _D_IN),
            (d_sae <= _MAX_D_SAE and d_sae % _MULT == 0, _D_SAE),
            (act != "topk" or 1 <= k <= _MAX_K, _K),
            # ghost gradients on a transcoder (transcoder.py:82-86: the ghost term sees the INPUT activation): equal widths, one process
            (not (tc and ghost) or (d_out == d_in and not self._mr),
             "ghost gradients on a transcoder with tokens sharded over ranks / d_out != d_in"),
            (kind is not None, "activation {cfg.activation_fn_str!r}"),
            # lp_norm > 1 in the sparsity term (sae.py:617) runs on the dense GEMMs' epilogues
            (kind != "relu" or float(getattr(sae, "lp_norm", 1)) >= 1.0,
             "lp_norm = {sae.lp_norm} (p < 1 has no finite gradient at zero activations: supported p >= 1)"),
            # hook points of DIFFERENT width: every row padded to the wider of the two (pv_sae_transcoder.d_in_true / d_out_true); the
            # reference's skip connection needs d_out == d_in
            (not tc or d_out == d_in or (sae._parameters.get("W_skip") is None and d_out % _MULT_DENSE == 0 and d_out <= _MAX_D_IN
                                         and d_in % _MULT_DENSE == 0), _TC_WIDTHS),
            (cfg.normalize_activations in ("layer_norm", "constant_norm_rescale", "none", None),
             "normalize_activations = {cfg.normalize_activations!r}"),
            (not (gated or kind == "relu") or (d_in % _MULT_DENSE == 0 and d_sae % _MULT_DENSE == 0), _DENSE_WIDTHS),
            (not ghost or d_in % _MULT_DENSE == 0, _GHOST_WIDTH),         # (pv_sae_topk_ghost, the ghost GEMMs of pv_sae_dense_step)
            (self._on_device(sae, x), "a parameter is not a contiguous fp32 CUDA tensor"),
        ]

    @staticmethod
    def _on_device(sae, x: Optional[torch.Tensor]) -> bool:
        """The device entry of ``_native_limits``: the step's input (when given) and every parameter on the GPU, in fp32."""
        return (x is None or x.is_cuda) and all(p.is_cuda and p.dtype == torch.float32       # (not .parameters(): no sync of lazily kept layouts)
                                                for p in sae._parameters.values() if p is not None)

    def _native_kind(self, sae, x: torch.Tensor) -> Optional[str]:
        """Which fused HIP step serves this SAE ("topk" / "relu" / "gated", see ``_native_limits``), or None: the PyTorch path."""
        if self._native_pref is False:
            return None
        kind, limits = self._native_limits(sae, x)
        return kind if all(holds for holds, _ in limits) else None

    def _native_ok(self, sae, x: torch.Tensor) -> bool:
        return self._native_kind(sae, x) is not None

    def _native_why_not(self, sae) -> str:
        """The one-time fallback warning's diagnosis: the conditions of ``_native_limits`` that do not hold."""
        return "; ".join(text.format(cfg=sae.cfg, sae=sae, k=sae.cfg.activation_fn_kwargs.get("k"), kind=type(sae).__name__)
                         for holds, text in self._native_limits(sae)[1] if not holds)

    def _get_engine(self, sae, n_tokens: int):
        from .native_sae import NativeSAE
        eng = self._engine
        tc_names = tuple(n for n in ("b_dec_out", "W_skip") if sae._parameters.get(n) is not None)
        stale = eng is not None and (any(eng.params[n].data_ptr() != sae._parameters[n].data_ptr()
                                         for n in ("W_enc", "W_dec", "b_enc", "b_dec") + tc_names
                                         + tuple(n for n in ("b_gate", "r_mag", "b_mag") if n in sae._parameters))     # e.g. b_dec.data re-bound by an init
                                     or tuple(n for n in ("b_dec_out", "W_skip") if n in eng.params) != tc_names)
        if eng is None or eng.max_tokens < n_tokens or stale:
            if self._mr and eng is None:
                # replicas must start from identical parameters (a per-rank b_dec initialisation, a different seed or a
                # caller-supplied module would otherwise never converge: every rank applies the same summed gradient).
                # Only at the FIRST creation, which every rank reaches in its first step: a later re-creation (a larger
                # batch, a re-bound parameter) is a per-rank event and must not contain a collective.
                import torch.distributed as dist
                for p in sae.parameters():
                    if p.data.is_contiguous():
                        dist.broadcast(p.data, src=0)
                    else:                                        # (a view of an earlier engine's padded storage: unequal-width transcoder)
                        tmp = p.data.contiguous()
                        dist.broadcast(tmp, src=0)
                        p.data.copy_(tmp)
            old = eng
            if old is not None:
                old.materialize_w_enc()                          # (the new engine derives its shadows from the parameter)
            P_ = dict(sae._parameters)
            tcw = None
            if self.is_transcoder and int(getattr(sae.cfg, "d_out", sae.cfg.d_in)) != int(sae.cfg.d_in):
                # rows padded to D = max(d_in, d_out): the engine owns the padded storage, the module's parameters become views of it
                # (W_enc / b_dec: leading rows; W_dec / b_dec_out: leading columns), so both sides see every update
                d_i, d_o = int(sae.cfg.d_in), int(sae.cfg.d_out)
                D = max(d_i, d_o)
                with torch.no_grad():
                    def padded(p, shape, sl):
                        buf = torch.zeros(shape, dtype=torch.float32, device=p.device)
                        buf[sl].copy_(p.data)
                        p.data = buf[sl]
                        return buf
                    P_["W_enc"] = padded(P_["W_enc"], (D, sae.cfg.d_sae), (slice(0, d_i),))
                    P_["b_dec"] = padded(P_["b_dec"], (D,), (slice(0, d_i),))
                    P_["W_dec"] = padded(P_["W_dec"], (sae.cfg.d_sae, D), (slice(None), slice(0, d_o)))
                    P_["b_dec_out"] = padded(P_["b_dec_out"], (D,), (slice(0, d_o),))
                tcw = (d_i, d_o)
            eng = NativeSAE(P_["W_enc"], P_["W_dec"], P_["b_enc"], P_["b_dec"],
                            k=sae.cfg.activation_fn_kwargs.get("k", 1),        # (the dense ReLU + L1 step has no k)
                            layer_norm=sae.cfg.normalize_activations,
                            max_tokens=max(n_tokens, self.cfg.train_batch_size // self.world),
                            **{n: P_[n] for n in tc_names}, **({"tc_widths": tcw} if tcw else {}),
                            **({"gated": {n: P_[n] for n in ("b_gate", "r_mag", "b_mag")},
                                "gated_topk": sae.cfg.activation_fn_str == "topk"} if "b_gate" in P_ else
                               {"activation": sae.cfg.activation_fn_str,
                                "lp_norm": float(getattr(sae, "lp_norm", 1)) if sae.cfg.activation_fn_str != "topk" else 1.0}))
            if old is not None and old.n_flat == eng.n_flat:             # keep the optimizer state across a re-bind
                eng.flat_m.copy_(old.flat_m)
                eng.flat_v.copy_(old.flat_v)
                eng.adam_step = old.adam_step
            if not self._mr and isinstance(sae, StandardSparseAutoencoder):
                # one process: nobody but the kernels reads W_enc between steps -- they read its transposed master -- so the
                # parameter's own layout is rewritten only when somebody asks for it (sae.W_enc, state_dict(), parameters())
                eng.lazy_w_enc = True
                object.__setattr__(sae, "_native_sync_fn", eng.materialize_w_enc)
            self._engine = eng
        return eng

    # ---- data-parallel plumbing ----------------------------------------------------------------------
    def _shard(self, d_sae: int):
        """This rank's feature rows, or None when the optimizer cannot be sharded evenly on 16-byte boundaries."""
        if not self._mr or d_sae % (4 * self.world) != 0:
            return None
        n = d_sae // self.world
        return self.rank * n, (self.rank + 1) * n

    def sync_parameters(self) -> None:
        """Data parallel only: make the module's parameters complete on this rank.  ``train_step`` returns while the
        all-gather of the other ranks' updated rows is still in flight (it overlaps the next harvest); the next
        ``train_step``, ``checkpoint`` and the end of ``run`` wait for it themselves -- call this before reading
        ``sae.W_enc`` / ``W_dec`` / ``b_enc`` in between."""
        self._dp_flush(materialize=True)

    def _dp_flush(self, materialize: bool = False) -> None:
        """Wait for the parameter all-gathers of the previous step and rebuild the other ranks' rows of W_enc / W_enc16T.
        materialize (sync_parameters / checkpoint / end of run; NOT the per-step call): also bring the module's parameters up to
        date with what the engines train -- the feature-parallel shards, the lazily kept layout of W_enc."""
        if materialize and self._engine is not None:
            self._engine.materialize_w_enc()                     # (single process: the lazily kept parameter layout of W_enc)
        if materialize and self._fp is not None and self._fp_dirty:         # feature parallel: gather the shards into the module
            P = self._fp.gather_parameters()
            with torch.no_grad():
                for n in ("W_enc", "W_dec", "b_enc", "b_dec"):
                    p = getattr(self.sparse_coder, n)
                    if p.shape != P[n].shape:                       # (released by drop_replicas: a fresh allocation)
                        p.data = torch.empty_like(P[n])
                    p.copy_(P[n])                                   # (not through .data: the version counter must move)
            eng = getattr(self.sparse_coder, "_engine", None)       # the module's own inference engine re-derives its shadows
            if eng is not None:
                eng.invalidate()
            self._fp_dirty = False
        if not self._pending:
            return
        for w in self._pending:
            w.wait()
        self._pending = []
        eng = self._engine
        j_lo, j_hi = self._shard(eng.d_sae)
        eng.sync_shadows(from_transposed=True, j_lo=0, j_hi=j_lo)
        eng.sync_shadows(from_transposed=True, j_lo=j_hi, j_hi=eng.d_sae)

    @staticmethod
    def _reduce_scatter_rows(dist, seg: torch.Tensor, j_lo: int, j_hi: int) -> None:
        """seg[j_lo:j_hi] <- sum over ranks; the other rows are left undefined."""
        mine = seg[j_lo:j_hi]
        if dist.get_backend() == "nccl":
            dist.reduce_scatter_tensor(mine, seg)                   # in place: output = this rank's chunk of the input
        else:
            out = torch.empty_like(mine)                            # gloo (tests): no aliasing guarantees
            dist.reduce_scatter_tensor(out, seg)
            mine.copy_(out)

    # ---- one step ---------------------------------------------------------------------------------
    def train_step(self, sparse_autoencoder, optimizer, scheduler, act_freq_scores, n_forward_passes_since_fired,
                   n_frac_active_tokens, layer_acts, n_training_steps, n_training_tokens):
        hp = sparse_autoencoder.cfg
        layers = hp.hook_point_layer if isinstance(hp.hook_point_layer, list) else [hp.hook_point_layer]
        layer_id = 0 if isinstance(hp.hook_point_layer, list) else layers.index(hp.hook_point_layer)
        self._target = None
        if self.is_transcoder:                                                   # train_sae.py:299-301
            sae_in, self._target = layer_acts[:, 0, :], layer_acts[:, 1, :]
        else:
            sae_in = layer_acts[:, layer_id, :]
        sparse_autoencoder.train()

        if (n_training_steps + 1) % self.cfg.feature_sampling_window == 0:     # train_sae.py:310-326
            feature_sparsity = act_freq_scores / n_frac_active_tokens
            self._log_feature_sparsity(feature_sparsity, n_training_steps)
            act_freq_scores = torch.zeros(hp.d_sae, device=hp.device)
            n_frac_active_tokens = 0

        kind = self._native_kind(sparse_autoencoder, sae_in)                     # the route, resolved here and nowhere below
        native = kind is not None
        if self._native_pref is True and not native:
            from .._native import NativeError
            raise NativeError("use_native(True): this SAE configuration / input is not served by the fused HIP step "
                              f"(activation {hp.activation_fn_str!r}, architecture {getattr(hp, 'architecture', 'standard')!r}, "
                              f"device {sae_in.device})")
        if not native and sae_in.is_cuda and self._native_pref is None and not self._warned_torch_path:
            # auto mode on a GPU: say ONCE why this run is not on the fused kernels (a silent PyTorch path is ~1000 x slower)
            self._warned_torch_path = True
            import warnings
            warnings.warn("vit_prisma_amd: VisionSAETrainer trains this SAE on the PyTorch path, not on the MI355X kernels: "
                          + self._native_why_not(sparse_autoencoder), stacklevel=2)
        if native:
            loss, mse_loss, l1_loss, l0 = self._native_step(kind, sparse_autoencoder, optimizer, scheduler, sae_in,
                                                            act_freq_scores, n_forward_passes_since_fired)
        else:
            loss, mse_loss, l1_loss, l0 = self._torch_step(sparse_autoencoder, optimizer, scheduler, sae_in,
                                                           act_freq_scores, n_forward_passes_since_fired)
        n_frac_active_tokens += sae_in.shape[0] * self.world
        self.last_step_native = native
        return loss, mse_loss, l1_loss, l0, act_freq_scores, n_forward_passes_since_fired, n_frac_active_tokens

    def _native_step(self, kind, sae, optimizer, scheduler, x, act_freq_scores, n_since_fired):
        """One step on the HIP kernels.  kind ("topk" / "relu" / "gated", from ``train_step``) picks the route: ``_step_feature_parallel``
        (multi-rank top-k of a plain SAE without ghost gradients, unless ``use_feature_parallel(False)``), ``_step_topk`` or
        ``_step_dense``; the routes differ in what lies between here and the epilogue, which is common."""
        lr = optimizer.param_groups[0]["lr"]
        ghost = bool(sae.cfg.use_ghost_grads) and sae.training
        fp = kind == "topk" and self._use_tp(sae) and not self.is_transcoder and not ghost
        if fp:
            out = self._step_feature_parallel(sae, x, lr, act_freq_scores, n_since_fired)
        else:
            self._dp_flush()                                    # parameters of the previous step must have landed
            eng = self._get_engine(sae, x.shape[0])
            # statistics tensors are the caller's: the kernels update them in place
            eng.act_freq_scores = act_freq_scores
            eng.n_fwd_since_fired = n_since_fired
            # train_sae.py:330-332: the mask of the ghost term is taken BEFORE this step's statistics
            # (none for a gated SAE; none for a transcoder with its tokens sharded, which _native_limits keeps off these steps)
            dead = None
            if ghost and kind != "gated" and not (self._mr and self.is_transcoder):
                dead = n_since_fired > sae.cfg.dead_feature_window
            if kind == "topk":
                self._step_topk(eng, x, lr, dead, act_freq_scores, n_since_fired)
            else:
                self._step_dense(eng, kind == "gated", float(sae.l1_coefficient), x, lr, dead, act_freq_scores, n_since_fired)
        optimizer._opt_called = True                            # the native apply IS the optimizer step
        scheduler.step()
        if fp:
            return out
        self._invalidate_inference_engine(sae)
        sc = eng.scalars.clone()
        return sc[0], sc[1], None if kind == "topk" else sc[4], sc[2]

    # ---- the pieces of a multi-rank step -----------------------------------------------------------
    def _global_mean(self, t: torch.Tensor, n_global: int) -> torch.Tensor:
        """Mean over the GLOBAL batch of what the loss is taken against (its normaliser, sae.py:145; a transcoder: the target's)."""
        import torch.distributed as dist
        bm = t.float().sum(dim=0)
        dist.all_reduce(bm)
        return bm / n_global

    @staticmethod
    def _ghost_global(eng, x: torch.Tensor, n_global: int):
        """``ghost_global`` of NativeSAE.topk_ghost / dense_step after a pass that left ``sae_out`` and the mse loss of this rank's tokens:
        the ghost term (sae.py:151-179) normalises by the residual's column mean and rescales by the mse loss of the WHOLE batch."""
        import torch.distributed as dist
        gl = torch.cat([(eng.sae_out[:x.shape[0]] - x).sum(dim=0), eng.scalars[1:2]])
        dist.all_reduce(gl)
        return gl[:eng.d_in] / n_global, gl[eng.d_in:], n_global

    def _pack_bucket(self, eng, n_scalars: int, gb_dec: bool):
        """The step's small bucket, filled: [gb_dec (d_in) |] fire counts (d_sae) | scalars[:n_scalars] (loss, mse, l0; the dense forms
        also -, l1, ghost, aux).  Packed BEFORE the gradient collective is issued, reduced after it (``_reduce_bucket``)."""
        lead, d_sae = eng.d_in if gb_dec else 0, eng.d_sae
        if self._small is None or self._small.numel() != lead + d_sae + n_scalars:
            self._small = torch.empty(lead + d_sae + n_scalars, dtype=torch.float32, device=eng.scalars.device)
        small = self._small
        if gb_dec:
            small[:lead].copy_(eng._g["b_dec"])
        small[lead:lead + d_sae].copy_(eng.fire_count)
        small[lead + d_sae:].copy_(eng.scalars[:n_scalars])
        return small, lead

    def _reduce_bucket(self, eng, bucket, act_freq_scores, n_since_fired) -> None:
        """One all-reduce of the packed bucket, then its parts go back where they came from: statistics and losses over the global batch."""
        import torch.distributed as dist
        small, lead = bucket
        dist.all_reduce(small)
        if lead:
            eng._g["b_dec"].copy_(small[:lead])
        n_scalars = small.numel() - lead - eng.d_sae
        eng.scalars[:n_scalars].copy_(small[lead + eng.d_sae:])
        eng.scalars[2] /= self.world                            # l0 is a mean over tokens
        self._count_firing(small[lead:lead + eng.d_sae], act_freq_scores, n_since_fired)

    @staticmethod
    def _count_firing(fire: torch.Tensor, act_freq_scores, n_since_fired) -> None:
        """train_sae.py:356-361 on the global batch (one process: the kernels do it, PV_SAE_UPDATE_STATS)."""
        n_since_fired += 1
        n_since_fired[fire > 0] = 0
        act_freq_scores += fire

    # ---- the routes ----------------------------------------------------------------------------------
    def _step_topk(self, eng, x, lr, dead, act_freq_scores, n_since_fired) -> None:
        """The k-sparse step (pv_sae_step) of a plain SAE or a Transcoder; dead: the ghost term's mask (pv_sae_topk_ghost) or None.
        Multi-rank: tokens sharded; the gradient rows reduce-scattered to the ranks that own them (module docstring), or -- a Transcoder
        (b_dec_out, W_skip beside the four tensors the row shards know), a d_sae that does not shard -- all-reduced for a replicated
        optimizer."""
        tgt = {"target": self._target} if eng.transcoder else {}
        if not self._mr:
            if dead is not None:
                # sae.py:151-179: the step with complete gradient buffers over a decoder renormalised in place (the ghost term reads
                # W_dec as it lies), then the ghost term's additions
                eng.renorm_decoder()
                eng.step(x, update_stats=True, renorm_decoder=False, sparse_grads=False, want_out=True, **tgt)
                eng.topk_ghost(x, dead)
                eng.grad_sqnorm()
            else:
                # set_decoder_norm_to_unit_norm is part of the step; one process = nobody but the step's own apply reads the
                # gradient buffers, so the rows of features that kept no token are neither zeroed nor read (PV_SAE_SPARSE_GRADS)
                eng.step(x, update_stats=True, renorm_decoder=True, sparse_grads=True, fused_sqnorm=True, **tgt)
                eng.grad_sqnorm(from_step=True)                 # clip_grad_norm_ (the gradient is as the step wrote it)
            eng.apply(lr, self.cfg.max_grad_norm)
            return
        import torch.distributed as dist
        n_global = x.shape[0] * self.world
        dp = dict(batch_mean=self._global_mean(self._target if eng.transcoder else x, n_global), n_global=n_global, update_stats=False)
        if dead is not None:
            eng.renorm_decoder()
            eng.step(x, renorm_decoder=False, want_out=True, **dp)
            eng.topk_ghost(x, dead, ghost_global=self._ghost_global(eng, x, n_global))
        else:
            eng.step(x, renorm_decoder=True, **dp, **tgt)
        shard = None if eng.transcoder else self._shard(eng.d_sae)
        bucket = self._pack_bucket(eng, 3, gb_dec=not eng.transcoder)
        if eng.transcoder:
            dist.all_reduce(eng.flat_g)
        elif shard is None:
            dist.all_reduce(eng.flat_g[:eng.n_flat - eng.d_in])  # replicated optimizer: every rank needs every row (gb_dec: the bucket)
        else:
            for name in ("W_encT", "W_dec", "b_enc"):
                self._reduce_scatter_rows(dist, eng._g[name], *shard)
        self._reduce_bucket(eng, bucket, act_freq_scores, n_since_fired)
        if shard is None:
            eng.grad_sqnorm()
            eng.apply(lr, self.cfg.max_grad_norm)
            return
        j_lo, j_hi = shard
        eng.grad_sqnorm_rows(j_lo, j_hi, include_b_dec=self.rank == 0)
        dist.all_reduce(eng.scalars[3:4])                       # the clip norm is over the GLOBAL gradient
        eng.apply(lr, self.cfg.max_grad_norm, j_lo, j_hi)       # this rank's rows (+ b_dec, identically everywhere)
        self._pending = [dist.all_gather_into_tensor(full, full[j_lo:j_hi], async_op=True)
                         for full in (eng.W_encT, eng.params["W_dec"], eng.params["b_enc"])]

    def _step_dense(self, eng, gated: bool, l1: float, x, lr, dead, act_freq_scores, n_since_fired) -> None:
        """ReLU + L1 (sae.py:617-626; also a ReLU Transcoder) on pv_sae_relu_step -- sparse where the batch allows it, the dense GEMMs
        otherwise: the GPU decides -- or pv_sae_dense_step (ghost gradients: exp(hidden_pre) of the dead columns is a dense quantity),
        or a Gated SAE on its own step.  Multi-rank: tokens sharded, ONE all-reduce of the flat gradient buffer and a replicated
        optimizer (the step is 6-11 ms of fp32 GEMMs: the 151 MB are not what bounds it), statistics and losses over the global batch
        like every other route."""
        tgt = {"target": self._target} if eng.transcoder else {}
        dp = dict(update_stats=True)
        if self._mr:
            import torch.distributed as dist
            n_global = x.shape[0] * self.world
            dp = dict(batch_mean=self._global_mean(self._target if eng.transcoder else x, n_global), n_global=n_global, update_stats=False)
        if gated and eng.gated_topk:
            eng.gated_topk_step(x, **dp)
        elif gated:
            eng.gated_step(x, l1, **dp)
        elif dead is not None:
            if self._mr:
                # the ghost term's two batch-wide quantities: a pass without it gives this rank's share of both, the step proper follows
                eng.dense_step(x, l1, want_out=True, renorm_decoder=True, **dp)
                dp["ghost_global"] = self._ghost_global(eng, x, n_global)
            eng.dense_step(x, l1, renorm_decoder=True, dead_mask=dead, **dp, **tgt)
        else:
            eng.relu_step(x, l1, renorm_decoder=True, sparse_grads=not self._mr, **dp, **tgt)
        if self._mr:
            bucket = self._pack_bucket(eng, 7, gb_dec=False)
            dist.all_reduce(eng.flat_g)                         # every rank's share of the gradient (scaled by 1 / N_global already)
            self._reduce_bucket(eng, bucket, act_freq_scores, n_since_fired)
        # clip_grad_norm_ over the whole (summed) gradient; one process: from the per-feature terms the step left
        eng.grad_sqnorm(from_step=not self._mr)
        eng.apply(lr, self.cfg.max_grad_norm)

    @staticmethod
    def _invalidate_inference_engine(sae) -> None:
        """The training kernels update the parameters through raw pointers (no version bump): the module's own inference
        engine (StandardSparseAutoencoder.forward / encode on the HIP path) must re-derive its shadows before its next use."""
        inf = sae.__dict__.get("_engine")
        if inf is not None:
            inf.invalidate()

    def _make_shard_engine(self, sae, max_tokens: int):
        """Engine over one rank's feature shard (tests substitute the CPU twin)."""
        from .native_sae import NativeSAE
        k, ln = sae.cfg.activation_fn_kwargs["k"], sae.cfg.normalize_activations
        return lambda We, Wd, be, bd: NativeSAE(We, Wd, be, bd, k=k, layer_norm=ln, max_tokens=max_tokens)

    def _step_feature_parallel(self, sae, x, lr, act_freq_scores, n_since_fired):
        """Feature-parallel step (sae/feature_parallel.py): every rank brings its tokens, all ranks see the global batch,
        each owns d_sae / world features for good."""
        import torch.distributed as dist
        from .feature_parallel import FeatureParallelSAE
        n_global = x.shape[0] * self.world
        if self._fp is None:
            for p in sae.parameters():                          # shards are cut from identical replicas
                dist.broadcast(p.data, src=0)
            self._fp = FeatureParallelSAE(sae.W_enc.data, sae.W_dec.data, sae.b_enc.data, sae.b_dec.data,
                                          sae.cfg.activation_fn_kwargs["k"], self._make_shard_engine(sae, n_global),
                                          dist=dist, rank=self.rank, world=self.world)
        fp = self._fp
        if self._fp_drop:                                       # the shards are the truth from here on: release the replicas
            for n in ("W_enc", "W_dec"):
                p = getattr(sae, n)
                if p.numel():
                    p.data = torch.empty(0, dtype=p.dtype, device=p.device)
        loss, l0 = fp.step(fp.gather_tokens(x), lr, self.cfg.max_grad_norm)
        self._fp_dirty = True
        self._count_firing(fp.fire_count, act_freq_scores, n_since_fired)
        return loss, loss, None, l0

    def _torch_step(self, sae, optimizer, scheduler, x, act_freq_scores, n_since_fired):
        """The reference algorithm on PyTorch autograd (CPU, ReLU/L1, ghost grads, ...)."""
        sae.set_decoder_norm_to_unit_norm()
        optimizer.zero_grad()
        dead = (n_since_fired > sae.cfg.dead_feature_window).bool()
        if self.is_transcoder:
            sae_out, feature_acts, loss, mse_loss, l1_loss, ghost, aux = sae(x, self._target, dead)
        else:
            sae_out, feature_acts, loss, mse_loss, l1_loss, ghost, aux = sae(x, dead)
        with torch.no_grad():
            fire = (feature_acts.abs() > 0).float().sum(0)
            pos = (feature_acts > 0).float().sum(-2)
            l0 = (feature_acts > 0).float().sum(-1).mean()
            if self.world > 1:                                   # statistics are over the GLOBAL batch, like the native path
                import torch.distributed as dist
                dist.all_reduce(fire)
                dist.all_reduce(pos)
                dist.all_reduce(l0)
                l0 = l0 / self.world
            n_since_fired += 1
            n_since_fired[pos > 0] = 0
            act_freq_scores += fire
        loss.backward()
        if self.world > 1:
            import torch.distributed as dist
            for p in sae.parameters():
                dist.all_reduce(p.grad)
                p.grad /= self.world
        if self.cfg.max_grad_norm:
            torch.nn.utils.clip_grad_norm_(sae.parameters(), max_norm=self.cfg.max_grad_norm)
        sae.remove_gradient_parallel_to_decoder_directions()
        optimizer.step()
        scheduler.step()
        return loss, mse_loss, l1_loss, l0

    # ---- logging / checkpoints --------------------------------------------------------------------
    def _log_feature_sparsity(self, feature_sparsity: torch.Tensor, n_training_steps: int) -> None:
        wb = _wandb()
        if self.cfg.log_to_wandb and wb is not None and self.rank == 0:
            log_sp = torch.log10(feature_sparsity + 1e-10).detach().cpu()
            wb.log({"metrics/mean_log10_feature_sparsity": log_sp.mean().item(),
                    "sparsity/below_1e-5": (feature_sparsity < 1e-5).float().mean().item(),
                    "sparsity/below_1e-6": (feature_sparsity < 1e-6).float().mean().item()}, step=n_training_steps)

    def checkpoint(self, sae, n_training_tokens, act_freq_scores, n_frac_active_tokens):
        self._dp_flush(materialize=True)
        if self.rank != 0:
            return
        folder = self.cfg.checkpoint_path
        os.makedirs(folder, exist_ok=True)
        self.cfg.save_config(os.path.join(folder, "config.json"))
        sae.set_decoder_norm_to_unit_norm()
        if self._engine is not None:                             # W_dec was edited between steps: 1 / ||row|| of the last apply is stale
            self._engine.invalidate()
        path = os.path.join(folder, f"n_images_{n_training_tokens // max(self.cfg.context_size, 1)}.pt")
        sae.save_model(path)
        sparsity = torch.log10(act_freq_scores / max(n_frac_active_tokens, 1) + 1e-10).detach().cpu()
        torch.save(sparsity, path.replace(".pt", "_log_feature_sparsity.pt"))

    # ---- the loop (train_sae.py:772-861) ----------------------------------------------------------
    def run(self):
        cfg = self.cfg
        wb = _wandb()
        if cfg.log_to_wandb and wb is None and self.rank == 0:
            print("[vit_prisma_amd] wandb is not installed: log_to_wandb ignored")
        (act_freq_scores, n_since_fired, n_frac_active_tokens, optimizer, scheduler) = self.initialize_training_variables()
        self.initialize_geometric_medians()
        n_training_steps = 0
        n_training_tokens = 0
        try:
            from tqdm import tqdm
            pbar = tqdm(total=cfg.total_training_tokens, desc="Training SAE", mininterval=20, disable=self.rank != 0)
        except Exception:
            pbar = None
        loss = mse_loss = l0 = None
        while n_training_tokens < cfg.total_training_tokens:
            layer_acts = self.activations_store.next_batch()
            (loss, mse_loss, l1_loss, l0, act_freq_scores, n_since_fired, n_frac_active_tokens) = self.train_step(
                sparse_autoencoder=self.sparse_coder, optimizer=optimizer, scheduler=scheduler, layer_acts=layer_acts,
                n_training_steps=n_training_steps, n_training_tokens=n_training_tokens, act_freq_scores=act_freq_scores,
                n_forward_passes_since_fired=n_since_fired, n_frac_active_tokens=n_frac_active_tokens)
            n_training_steps += 1
            n_training_tokens += layer_acts.shape[0] * self.world
            if self.checkpoint_thresholds and n_training_tokens > self.checkpoint_thresholds[0]:
                self.checkpoint(self.sparse_coder, n_training_tokens, act_freq_scores, n_frac_active_tokens)
                self.checkpoint_thresholds.pop(0)
            if pbar is not None:
                pbar.update(layer_acts.shape[0] * self.world)
                if n_training_steps % 50 == 0:        # .item() syncs the stream: keep it off the hot loop
                    pbar.set_description(f"Training SAE: Loss: {float(loss):.4f}, MSE Loss: {float(mse_loss):.4f}, "
                                         f"L0: {float(l0):.4f}", refresh=False)
        self._dp_flush(materialize=True)
        if cfg.n_checkpoints:
            self.checkpoint(self.sparse_coder, n_training_tokens, act_freq_scores, n_frac_active_tokens)
        if pbar is not None:
            pbar.close()
        self.final_stats = dict(loss=None if loss is None else float(loss), n_training_steps=n_training_steps,
                                n_training_tokens=n_training_tokens)
        return self.sparse_coder
