"""Which engine calls and which collectives each native route of ``VisionSAETrainer.train_step`` issues, in order.

A recording engine stands in for ``NativeSAE`` (every method call is logged, nothing is computed) and, for the multi-rank routes,
recorders stand in for the collectives of ``torch.distributed`` (world 2, rank 0, no process group).  Each route runs two
``train_step`` calls and ``sync_parameters()``; the log is compared with the literal table below.  Engine calls are bound to
``NativeSAE``'s own signatures and written with the arguments that differ from its defaults, tensors by role and shape;
``batch_mean`` is also compared by value with the column sum over the global token count.  What the steps compute is the business
of tests/test_dp_sharded_cpu.py (gloo, the CPU twin) and tests/test_native_sae_gpu.py (the kernels)."""
import functools
import inspect

import pytest
import torch
import torch.distributed as dist

from vit_prisma_amd.sae import VisionModelSAERunnerConfig, VisionSAETrainer
from vit_prisma_amd.sae.native_sae import NativeSAE

K, N = 4, 8


class RecordingEngine:
    """NativeSAE's attributes as far as the trainer reads them; every method call lands in ``log``."""

    def __init__(self, log, d_in, d_sae, max_tokens, transcoder=False, gated_topk=False):
        self.log, self.d_in, self.d_sae, self.k, self.max_tokens = log, d_in, d_sae, K, max_tokens
        self.transcoder, self.gated_topk = transcoder, gated_topk
        nW = d_in * d_sae
        self.n_flat = 2 * nW + d_sae + d_in
        self.flat_g = torch.zeros(self.n_flat)
        self._g = dict(W_encT=self.flat_g[:nW].view(d_sae, d_in), W_dec=self.flat_g[nW:2 * nW].view(d_sae, d_in),
                       b_enc=self.flat_g[2 * nW:2 * nW + d_sae], b_dec=self.flat_g[2 * nW + d_sae:])
        self.W_encT = torch.zeros(d_sae, d_in)
        self.params = dict(W_dec=torch.zeros(d_sae, d_in), b_enc=torch.zeros(d_sae))
        self.scalars = torch.arange(8, dtype=torch.float32)
        self.fire_count = torch.zeros(d_sae)
        self.sae_out = torch.zeros(max_tokens, d_in)
        self.named = {}                                               # role -> tensor (the step's input and target), set by the test
        self._bm = None

    def __getattr__(self, name):                                     # (only what __init__ did not set: the methods)
        if name.startswith("__"):
            raise AttributeError(name)
        return lambda *a, **kw: self.log.append(self._describe(name, a, kw))

    def _arg(self, v):
        if isinstance(v, torch.Tensor):
            # (the trainer hands on views it takes itself: roles go by storage, shape and strides)
            role = "batch_mean" if v is self._bm else next(
                (n for n, ref in self.named.items() if ref is not None and v.data_ptr() == ref.data_ptr() and v.shape == ref.shape
                 and v.stride() == ref.stride()), "bool" if v.dtype == torch.bool else "f32")
            return f"{role}{list(v.shape)}"
        if isinstance(v, tuple):
            return "(" + ", ".join(self._arg(e) for e in v) + ")"
        return repr(v)

    def _describe(self, name, a, kw):
        sig = _signature(name)
        bound = sig.bind(self, *a, **kw)
        bound.apply_defaults()
        if isinstance(bound.arguments.get("batch_mean"), torch.Tensor):
            self._bm = bound.arguments["batch_mean"]
            assert torch.equal(self._bm, self.want_batch_mean), "batch_mean is not the column sum over n_global"
        shown = [f"{n}={self._arg(v)}" for n, v in bound.arguments.items()
                 if n != "self" and not (sig.parameters[n].default is not inspect.Parameter.empty and _same(v, sig.parameters[n].default))]
        return f"{name}({', '.join(shown)})"


@functools.lru_cache(maxsize=None)
def _signature(name):
    return inspect.signature(getattr(NativeSAE, name))


def _same(v, default):
    return not isinstance(v, torch.Tensor) and v == default and type(v) is type(default)


class _Work:
    def __init__(self, log):
        self.log = log

    def wait(self):
        self.log.append("wait")


def _patch_collectives(monkeypatch, log):
    def shapes(*ts):
        return " <- ".join(str(list(t.shape)) for t in ts)

    monkeypatch.setattr(dist, "all_reduce", lambda t, *a, **kw: log.append(f"all_reduce {shapes(t)}"))
    monkeypatch.setattr(dist, "broadcast", lambda t, *a, **kw: log.append(f"broadcast {shapes(t)}"))
    monkeypatch.setattr(dist, "reduce_scatter_tensor", lambda out, inp, *a, **kw: log.append(f"reduce_scatter_tensor {shapes(out, inp)}"))
    monkeypatch.setattr(dist, "get_backend", lambda *a, **kw: "nccl")

    def all_gather(out, inp, async_op=False, **kw):
        log.append(f"all_gather_into_tensor {shapes(out, inp)}" + (" async" if async_op else ""))
        return _Work(log)

    monkeypatch.setattr(dist, "all_gather_into_tensor", all_gather)


# ---- the table: route -> (the log of one step, what the SECOND step logs before it, what sync_parameters() logs after it) ----
APPLY = ["apply(lr=0.001, max_grad_norm=1.0)"]
MEAN = ["all_reduce [16]"]                                            # the global batch mean, before the forward
DP = "batch_mean=batch_mean[16], n_global=16, update_stats=False"
FLAT = ["all_reduce [2128]"]                                          # the flat gradient buffer (2 x 16 x 64 + 64 + 16)
WAITS = ["wait", "wait", "wait", "sync_shadows(from_transposed=True, j_hi=0)", "sync_shadows(from_transposed=True, j_lo=32, j_hi=64)"]
SYNC = ["materialize_w_enc()"]
ROUTES = {
    # ---- one process
    "topk": (["step(x=x[8, 16], renorm_decoder=True, sparse_grads=True, fused_sqnorm=True)", "grad_sqnorm(from_step=True)"] + APPLY, [], SYNC),
    "topk_ghost": (["renorm_decoder()", "step(x=x[8, 16], want_out=True)", "topk_ghost(x=x[8, 16], dead_mask=bool[64])",
                    "grad_sqnorm()"] + APPLY, [], SYNC),
    "topk_tc": (["step(x=x[8, 16], renorm_decoder=True, sparse_grads=True, target=target[8, 16], fused_sqnorm=True)",
                 "grad_sqnorm(from_step=True)"] + APPLY, [], SYNC),
    "relu": (["relu_step(x=x[8, 16], l1_coefficient=0.002, sparse_grads=True)", "grad_sqnorm(from_step=True)"] + APPLY, [], SYNC),
    "relu_ghost": (["dense_step(x=x[8, 16], l1_coefficient=0.002, dead_mask=bool[64])", "grad_sqnorm(from_step=True)"] + APPLY, [], SYNC),
    "gated": (["gated_step(x=x[8, 16], l1_coefficient=0.002)", "grad_sqnorm(from_step=True)"] + APPLY, [], SYNC),
    "gated_topk": (["gated_topk_step(x=x[8, 16])", "grad_sqnorm(from_step=True)"] + APPLY, [], SYNC),
    # ---- world 2, rank 0
    "w2_topk_sharded": (MEAN + [f"step(x=x[8, 16], {DP}, renorm_decoder=True)"]
                        + ["reduce_scatter_tensor [32, 16] <- [64, 16]"] * 2 + ["reduce_scatter_tensor [32] <- [64]", "all_reduce [83]",
                           "grad_sqnorm_rows(j_lo=0, j_hi=32, include_b_dec=True)", "all_reduce [1]",
                           "apply(lr=0.001, max_grad_norm=1.0, j_hi=32)"]
                        + ["all_gather_into_tensor [64, 16] <- [32, 16] async"] * 2 + ["all_gather_into_tensor [64] <- [32] async"],
                        WAITS, SYNC + WAITS),
    "w2_topk_replicated": (["all_reduce [20]", "step(x=x[8, 20], batch_mean=batch_mean[20], n_global=16, update_stats=False, renorm_decoder=True)",
                            "all_reduce [2460]", "all_reduce [83]", "grad_sqnorm()"] + APPLY, [], SYNC),
    "w2_topk_ghost": (MEAN + ["renorm_decoder()", f"step(x=x[8, 16], {DP}, want_out=True)", "all_reduce [17]",
                              "topk_ghost(x=x[8, 16], dead_mask=bool[64], ghost_global=(f32[16], f32[1], 16))"]
                      + ["reduce_scatter_tensor [32, 16] <- [64, 16]"] * 2 + ["reduce_scatter_tensor [32] <- [64]", "all_reduce [83]",
                         "grad_sqnorm_rows(j_lo=0, j_hi=32, include_b_dec=True)", "all_reduce [1]",
                         "apply(lr=0.001, max_grad_norm=1.0, j_hi=32)"]
                      + ["all_gather_into_tensor [64, 16] <- [32, 16] async"] * 2 + ["all_gather_into_tensor [64] <- [32] async"],
                      WAITS, SYNC + WAITS),
    "w2_topk_tc": (MEAN + [f"step(x=x[8, 16], {DP}, renorm_decoder=True, target=target[8, 16])"] + FLAT
                   + ["all_reduce [67]", "grad_sqnorm()"] + APPLY, [], SYNC),
    "w2_relu": (MEAN + [f"relu_step(x=x[8, 16], l1_coefficient=0.002, {DP})"] + FLAT + ["all_reduce [71]", "grad_sqnorm()"] + APPLY, [], SYNC),
    "w2_relu_ghost": (MEAN + [f"dense_step(x=x[8, 16], l1_coefficient=0.002, {DP}, want_out=True)", "all_reduce [17]",
                              f"dense_step(x=x[8, 16], l1_coefficient=0.002, {DP}, dead_mask=bool[64], ghost_global=(f32[16], f32[1], 16))"]
                      + FLAT + ["all_reduce [71]", "grad_sqnorm()"] + APPLY, [], SYNC),
    "w2_gated": (MEAN + [f"gated_step(x=x[8, 16], l1_coefficient=0.002, {DP})"] + FLAT + ["all_reduce [71]", "grad_sqnorm()"] + APPLY, [], SYNC),
    "w2_gated_topk": (MEAN + [f"gated_topk_step(x=x[8, 16], {DP})"] + FLAT + ["all_reduce [71]", "grad_sqnorm()"] + APPLY, [], SYNC),
}


@pytest.mark.parametrize("route", list(ROUTES))
def test_route_issues_these_engine_calls_and_collectives(route, monkeypatch):
    multi, name = route.startswith("w2_"), route[3:] if route.startswith("w2_") else route
    d_in, ef = (20, 3) if name == "topk_replicated" else (16, 4)      # (d_sae = 60: no multiple of 4 x world, _shard gives None)
    d_sae = d_in * ef
    gated, tc, ghost = name.startswith("gated"), name == "topk_tc", name.endswith("ghost")
    topk = name.startswith("topk") or name == "gated_topk"
    cfg = VisionModelSAERunnerConfig(
        hook_point_layer=1, layer_subtype="hook_resid_post", d_in=d_in, expansion_factor=ef, activation_fn_str="topk" if topk else "relu",
        activation_fn_kwargs={"k": K} if topk else {}, l1_coefficient=2e-3, normalize_activations="layer_norm", b_dec_init_method="mean",
        train_batch_size=N, lr=1e-3, max_grad_norm=1.0, _device="cpu", log_to_wandb=False, lr_scheduler_name="constant", n_checkpoints=0,
        use_ghost_grads=ghost, dead_feature_window=1, **(dict(architecture="gated") if gated else {}),
        **(dict(is_transcoder=True, transcoder_with_skip_connection=True, d_out=d_in, out_hook_point_layer=1) if tc else {}))
    tr = VisionSAETrainer(cfg, model=None, dataset=None).use_feature_parallel(False)
    sae = tr.sparse_coder
    log = []
    eng = RecordingEngine(log, d_in, d_sae, N, transcoder=tc, gated_topk=name == "gated_topk")
    tr._native_kind = lambda *a, **k: "gated" if gated else "topk" if topk else "relu"

    def get_engine(s, n_tokens):
        tr._engine = eng
        return eng

    tr._get_engine = get_engine
    if multi:
        tr.world, tr.rank = 2, 0
        _patch_collectives(monkeypatch, log)
    want_step, want_before_second, want_sync = ROUTES[route]
    act, since, frac, opt, sched = tr.initialize_training_variables()
    since[::3] = 5.0                                                  # (ghost routes: a third of the features count as dead)
    gen = torch.Generator().manual_seed(0)
    for t in range(2):
        acts = torch.randn(N, 2 if tc else 1, d_in, generator=gen)
        x, target = acts[:, 0, :], acts[:, 1, :] if tc else None
        eng.named = {"x": x, "target": target}
        eng.want_batch_mean = (target if tc else x).float().sum(dim=0) / (N * tr.world)
        del log[:]
        out = tr.train_step(sparse_autoencoder=sae, optimizer=opt, scheduler=sched, act_freq_scores=act, n_forward_passes_since_fired=since,
                            n_frac_active_tokens=frac, layer_acts=acts, n_training_steps=t, n_training_tokens=t * N * tr.world)
        loss, mse, l1, l0, act, since, frac = out
        assert tr.last_step_native and tr._engine is eng
        assert log == (want_before_second if t else []) + want_step, (t, log)
        assert eng.act_freq_scores is act and eng.n_fwd_since_fired is since        # the statistics tensors are the caller's
        # the returned scalars are copies of loss, mse, l1 (dense forms only), l0 in the engine's order
        assert (float(loss), float(mse), float(l0)) == (0.0, 1.0, 2.0 / tr.world if multi else 2.0)
        assert l1 is None if (topk and not gated) else float(l1) == 4.0
        assert frac == (t + 1) * N * tr.world and opt._opt_called
        eng.scalars.copy_(torch.arange(8, dtype=torch.float32))
    assert len(tr._pending) == (3 if name in ("topk_sharded", "topk_ghost") and multi else 0)
    del log[:]
    tr.sync_parameters()
    assert log == want_sync and not tr._pending



# ---- the limits of the native steps: (cfg arguments, the kind VisionSAETrainer._native_kind gives on a GPU, the sentence
# _native_why_not must hold).  Sentences marked NEW name a condition the diagnosis was silent about before (it fell back to the
# sentence about the parameters' device); the others are its long-standing texts, word for word.
FALLBACK = "a parameter is not a contiguous fp32 CUDA tensor"
TC = dict(is_transcoder=True, out_hook_point_layer=1)
LIMITS = {
    "topk": (dict(d_in=64), "topk", None),
    "topk_d_in_68": (dict(d_in=68), "topk", None),                                   # (a multiple of 4 serves the k-sparse step)
    "topk_d_in_66": (dict(d_in=66), None, "d_in = 66 (supported: multiples of 4 up to 1280 = ViT-H/14)"),
    "topk_d_in_1284": (dict(d_in=1284), None, "d_in = 1284 (supported: multiples of 4 up to 1280 = ViT-H/14)"),
    "topk_d_sae_65600": (dict(d_in=16, expansion_factor=4100), None, "d_sae = 65600 (supported: multiples of 4 up to 65536)"),
    "topk_k_0": (dict(d_in=64, k=0), None, "k = 0 (supported: 1..256)"),
    "topk_k_256": (dict(d_in=64, k=256), "topk", None),
    "topk_k_257": (dict(d_in=64, k=257), None, "k = 257 (supported: 1..256)"),
    "topk_lp_half": (dict(d_in=64, lp_norm=0.5), "topk", None),                      # (no sparsity term on the top-k step)
    "topk_ghost": (dict(d_in=64, use_ghost_grads=True), "topk", None),
    "topk_ghost_d_in_68": (dict(d_in=68, use_ghost_grads=True), None, "ghost gradients with d_in = 68 (supported: multiples of 8)"),   # NEW
    "relu": (dict(d_in=64, act="relu"), "relu", None),
    "tanh_relu": (dict(d_in=64, act="tanh-relu"), "relu", None),
    "gelu": (dict(d_in=64, act="relu", then="gelu"), None, "activation 'gelu'"),      # (no module of it: the cfg is edited after)
    "relu_d_in_68": (dict(d_in=68, act="relu"), None, "d_in = 68, d_sae = 544 (the ReLU + L1 and the gated steps: multiples of 8)"),  # NEW
    "relu_lp_half": (dict(d_in=64, act="relu", lp_norm=0.5), None,
                     "lp_norm = 0.5 (p < 1 has no finite gradient at zero activations: supported p >= 1)"),
    "gated": (dict(d_in=64, act="relu", architecture="gated"), "gated", None),
    "gated_topk": (dict(d_in=64, architecture="gated"), "gated", None),
    "gated_k_257": (dict(d_in=64, k=257, architecture="gated"), None, "k = 257 (supported: 1..256)"),
    "gated_tanh_relu": (dict(d_in=64, act="tanh-relu", architecture="gated"), None, "activation 'tanh-relu'"),                      # NEW
    "gated_d_in_68": (dict(d_in=68, act="relu", architecture="gated"), None,
                      "d_in = 68, d_sae = 544 (the ReLU + L1 and the gated steps: multiples of 8)"),                                # NEW
    "tc": (dict(d_in=64, d_out=64, transcoder_with_skip_connection=True, **TC), "topk", None),
    "tc_wider": (dict(d_in=64, d_out=128, transcoder_with_skip_connection=False, **TC), "topk", None),
    "tc_wider_skip": (dict(d_in=64, d_out=128, transcoder_with_skip_connection=True, **TC), None,
                      "a transcoder with d_out != d_in and the skip connection / widths that are not multiples of 8 / d_out > 1280"),
    "tc_wider_ghost": (dict(d_in=64, d_out=128, transcoder_with_skip_connection=False, use_ghost_grads=True, **TC), None,
                       "ghost gradients on a transcoder with tokens sharded over ranks / d_out != d_in"),
}


@pytest.mark.parametrize("case", list(LIMITS))
def test_native_kind_and_its_diagnosis_read_one_list_of_limits(case):
    kw, want_kind, want_text = LIMITS[case]
    kw = dict(kw)
    act, k, then = kw.pop("act", "topk"), kw.pop("k", 8), kw.pop("then", None)
    cfg = VisionModelSAERunnerConfig(
        hook_point_layer=1, layer_subtype="hook_resid_post", activation_fn_str=act, activation_fn_kwargs={"k": k} if act == "topk" else {},
        normalize_activations="layer_norm", b_dec_init_method="mean", train_batch_size=N, _device="cpu", log_to_wandb=False,
        lr_scheduler_name="constant", n_checkpoints=0, **{"expansion_factor": 8, **kw})
    tr = VisionSAETrainer(cfg, model=None, dataset=None)
    sae, x = tr.sparse_coder, torch.zeros(N, cfg.d_in)
    if then is not None:
        cfg.activation_fn_str = then
    tr._target = x if tr.is_transcoder else None                      # (train_step splits a transcoder's target off the batch)
    assert tr._native_kind(sae, x) is None and not tr._native_ok(sae, x)            # a CPU takes the PyTorch path
    on_cpu = tr._native_why_not(sae)
    assert on_cpu.endswith(FALLBACK) and (on_cpu == FALLBACK) == (want_kind is not None)
    tr._on_device = lambda *a: True                                   # ... and with the device entry taken as satisfied:
    assert tr._native_kind(sae, x) == want_kind and tr._native_ok(sae, x) == (want_kind is not None)
    why = tr._native_why_not(sae)
    assert FALLBACK not in why and (why != "") == (want_kind is None)
    assert want_text is None or want_text in why.split("; ")
    assert tr.use_native(False)._native_kind(sae, x) is None
