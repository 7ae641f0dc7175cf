"""Drop-in loose ends (north_star: "existing Prisma notebooks and SAE configs drop in unchanged"):
  * ``vit_prisma_amd.install_as("vit_prisma")``: the reference's import paths resolve to this build
  * checkpoints written by the reference (pickled vit_prisma.sae.config.VisionModelSAERunnerConfig) load, in the
    reference's argument order, and reproduce the reference module's output bit for bit
  * VisionSAETrainer.run() end to end on the tiny model, geometric-median b_dec initialisation against the reference's
    own result
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from vit_prisma_amd import HookedViT, HookedViTConfig
from vit_prisma_amd.sae import StandardSparseAutoencoder, VisionModelSAERunnerConfig, VisionSAETrainer
from vit_prisma_amd.sae.geometric_median import compute_geometric_median
from vit_prisma_amd.synth import ARCHS, synth_images, synth_vit_state

from conftest import GOLDEN, ROOT


def test_import_aliases_cover_the_reference_paths():
    code = (
        "import vit_prisma_amd as A; A.install_as('vit_prisma')\n"
        "from vit_prisma.models.base_vit import HookedViT\n"
        "from vit_prisma.configs.HookedViTConfig import HookedViTConfig\n"
        "from vit_prisma.prisma_tools.hook_point import HookPoint\n"
        "from vit_prisma.prisma_tools.hooked_root_module import HookedRootModule\n"
        "from vit_prisma.prisma_tools.activation_cache import ActivationCache\n"
        "from vit_prisma.sae.config import VisionModelSAERunnerConfig\n"
        "from vit_prisma.sae.sae import StandardSparseAutoencoder, GatedSparseAutoencoder, SparseAutoencoder\n"
        "from vit_prisma.sae.transcoder import Transcoder\n"
        "from vit_prisma.sae.train_sae import VisionSAETrainer\n"
        "from vit_prisma.sae.training.activations_store import VisionActivationsStore, CacheVisionActivationStore\n"
        "from vit_prisma.sae.training.geometric_median import compute_geometric_median\n"
        "from vit_prisma.sae import VisionSAETrainer as T2\n"
        "assert HookedViT is A.HookedViT and T2 is VisionSAETrainer\n"
        "import vit_prisma.sae.sae as m; assert m.StandardSparseAutoencoder.__module__ == 'vit_prisma_amd.sae.sae'\n"
        "print('aliases ok')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0 and "aliases ok" in r.stdout, r.stderr[-2000:]


_CKPT_CHECK = """
import os, sys, torch
from vit_prisma_amd.sae import StandardSparseAutoencoder, VisionModelSAERunnerConfig
d = sys.argv[1]
io = torch.load(os.path.join(d, "io.pt"))
m = StandardSparseAutoencoder.load_from_pretrained(os.path.join(d, "ref_legacy.pt"))
assert type(m.cfg) is VisionModelSAERunnerConfig and m.cfg.d_sae == 512 and m.cfg.activation_fn_kwargs == {"k": 8}
assert torch.equal(m(io["x"])[0], io["out"])
# split form: bare state dict + config.json beside it; the reference's positional order (weights_path, current_cfg)
m2 = StandardSparseAutoencoder.load_from_pretrained(os.path.join(d, "weights.pt"), {"lr": 0.5, "not_a_field": 1})
assert m2.cfg.lr == 0.5 and not hasattr(m2.cfg, "not_a_field") and torch.equal(m2(io["x"])[0], io["out"])
m3 = StandardSparseAutoencoder.load_from_pretrained(os.path.join(d, "weights.pt"), config_path=os.path.join(d, "config.json"))
assert torch.equal(m3(io["x"])[0], io["out"])
try:
    StandardSparseAutoencoder.load_from_pretrained(os.path.join(d, "nope.pt"))
    raise SystemExit("no FileNotFoundError")
except FileNotFoundError:
    pass
print("checkpoints ok")
"""


def test_checkpoints_written_by_the_reference_load_and_reproduce_its_output():
    """Bit for bit against the reference module's reconstruction (io.pt), which was computed with MKL's conditional numerical
    reproducibility: the same setting here (in a fresh process: MKL reads it once) gives the same bits on any x86 CPU, where the
    default code paths differ in the last bit between instruction sets."""
    env = dict(os.environ, MKL_CBWR="COMPATIBLE", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", _CKPT_CHECK, os.path.join(GOLDEN, "sae_ref_ckpt")], capture_output=True, text=True,
                       cwd=ROOT, env=env, timeout=300)
    assert r.returncode == 0 and "checkpoints ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_geometric_median_equals_the_references():
    g = np.load(os.path.join(GOLDEN, "geometric_median.npz"))
    res = compute_geometric_median(torch.from_numpy(g["points"]), maxiter=100)
    assert float((res.median - torch.from_numpy(g["median"])).abs().max()) < 1e-5
    assert float((res.median - torch.from_numpy(g["points"]).mean(0)).norm()) > 1.0       # it is not the mean


@pytest.mark.parametrize("b_dec_init", ["geometric_median", "mean"])
def test_trainer_run_end_to_end_on_the_tiny_model(tmp_path, b_dec_init):
    """VisionSAETrainer.run() (train_sae.py:772-861): store harvest -> b_dec initialisation -> ~20 train steps ->
    checkpoint, on CPU with the tiny ViT; the loss must fall and the checkpoint must load back."""
    arch = ARCHS["tiny"]
    vit = HookedViT(HookedViTConfig(**arch, device="cpu"))
    vit.load_state_dict({k: torch.from_numpy(v) for k, v in synth_vit_state(arch, 0).items()})
    vit.eval()
    images = torch.from_numpy(synth_images(arch, 64, 3))
    ds = [(images[i], 0) for i in range(64)]
    n_steps, bs = 20, 128
    cfg = VisionModelSAERunnerConfig(
        hook_point_layer=1, layer_subtype="hook_resid_post", d_in=64, expansion_factor=4, activation_fn_str="topk",
        activation_fn_kwargs={"k": 8}, normalize_activations="layer_norm", b_dec_init_method=b_dec_init, train_batch_size=bs,
        lr=2e-3, max_grad_norm=1.0, _device="cpu", log_to_wandb=False, lr_scheduler_name="constant", n_checkpoints=1,
        context_size=17, store_batch_size=8, n_batches_in_buffer=4, checkpoint_path=str(tmp_path), verbose=False)
    cfg.total_training_images = n_steps * bs // 17 + 1
    tr = VisionSAETrainer(cfg, vit, ds, eval_dataset=ds)
    before = tr.sparse_coder.b_dec.detach().clone()
    losses = []
    orig = tr.train_step

    def spy(**kw):
        out = orig(**kw)
        losses.append(float(out[0]))
        return out

    tr.train_step = spy
    sae = tr.run()
    assert sae is tr.sparse_coder and len(losses) >= n_steps and tr.final_stats["n_training_steps"] == len(losses)
    assert not torch.equal(sae.b_dec.detach(), before)                         # b_dec was initialised from the buffer
    assert np.mean(losses[-3:]) < np.mean(losses[:3])
    ck = [f for f in os.listdir(cfg.checkpoint_path) if f.endswith(".pt") and "sparsity" not in f]
    assert ck and os.path.exists(os.path.join(cfg.checkpoint_path, "config.json"))
    back = StandardSparseAutoencoder.load_from_pretrained(os.path.join(cfg.checkpoint_path, ck[0]))
    assert torch.allclose(back.W_dec, sae.W_dec) and float((back.W_dec.norm(dim=1) - 1).abs().max()) < 1e-5


def test_load_hooked_model_offline_from_a_local_open_clip_checkpoint(tmp_path):
    """The notebook entry point (models/model_loader.py:278-368) through the ``vit_prisma`` alias: config from the architecture table of
    the named model, weights from a LOCAL open_clip checkpoint (the build has no network), same forward as a HookedViT loaded by hand."""
    import torch
    import vit_prisma_amd
    from vit_prisma_amd.synth import ARCHS, synth_vit_state
    vit_prisma_amd.install_as("vit_prisma", force=True)
    try:
        from vit_prisma.models.model_loader import load_hooked_model, list_available_models
        name = "open-clip:laion/CLIP-ViT-B-32-DataComp.XL-s13B-b90K"
        assert name in list_available_models()
        arch = ARCHS["clip-vit-b32"]
        # an open_clip-layout checkpoint of the B/32 shape (random values), written to disk
        g = torch.Generator().manual_seed(0)
        d, L, p, T, ncls = arch["d_model"], arch["n_layers"], arch["patch_size"], 50, arch["n_classes"]
        sd = {"visual.class_embedding": torch.randn(d, generator=g) * 0.1, "visual.positional_embedding": torch.randn(T, d, generator=g) * 0.1,
              "visual.conv1.weight": torch.randn(d, 3, p, p, generator=g) * 0.02, "visual.ln_pre.weight": torch.ones(d), "visual.ln_pre.bias": torch.zeros(d),
              "visual.ln_post.weight": torch.ones(d), "visual.ln_post.bias": torch.zeros(d), "visual.proj": torch.randn(d, ncls, generator=g) * 0.03}
        for l in range(L):
            o = f"visual.transformer.resblocks.{l}"
            sd.update({o + ".attn.in_proj_weight": torch.randn(3 * d, d, generator=g) * 0.03, o + ".attn.in_proj_bias": torch.zeros(3 * d),
                       o + ".attn.out_proj.weight": torch.randn(d, d, generator=g) * 0.03, o + ".attn.out_proj.bias": torch.zeros(d),
                       o + ".ln_1.weight": torch.ones(d), o + ".ln_1.bias": torch.zeros(d), o + ".ln_2.weight": torch.ones(d), o + ".ln_2.bias": torch.zeros(d),
                       o + ".mlp.c_fc.weight": torch.randn(4 * d, d, generator=g) * 0.03, o + ".mlp.c_fc.bias": torch.zeros(4 * d),
                       o + ".mlp.c_proj.weight": torch.randn(d, 4 * d, generator=g) * 0.03, o + ".mlp.c_proj.bias": torch.zeros(d)})
        path = str(tmp_path / "open_clip_b32.pt")
        torch.save(sd, path)
        model = load_hooked_model(name, device="cpu", local_path=path)
        assert type(model).__name__ == "HookedViT" and model.cfg.n_layers == 12 and model.cfg.d_model == 768 and model.cfg.model_name == name
        assert torch.equal(model.blocks[3].mlp.W_in, sd["visual.transformer.resblocks.3.mlp.c_fc.weight"].t())
        x = torch.randn(2, 3, 224, 224, generator=g)
        with torch.no_grad():
            out, cache = model.run_with_cache(x)
        assert out.shape == (2, 512) and len(cache) == 214
        import pytest
        with pytest.raises(FileNotFoundError):
            load_hooked_model(name, device="cpu")                                   # pretrained weights cannot be downloaded here
        rnd = load_hooked_model("openai/clip-vit-large-patch14-336", device="cpu", pretrained=False, dtype="bfloat16")
        assert rnd.cfg.n_layers == 24 and rnd.cfg.dtype == torch.bfloat16 and next(rnd.parameters()).dtype == torch.bfloat16
    finally:
        from vit_prisma_amd.compat import uninstall
        uninstall("vit_prisma")


def test_offline_loader_configs_carry_the_reference_registry_overrides():
    """Every model name the offline loader knows resolves to the config fields the reference's registry lays over the downloaded
    config (models/model_config_registry.py, applied by its load_config :201-203) -- read out of the reference into
    tests/golden/model_registry.json by gen_golden_model_registry.py.  Round-4 advisor finding: 'openai/clip-vit-base-patch32'
    came back with the open_clip B/32 values (eps 1e-5, L2-normalised output) instead of its own (1e-6, not normalised)."""
    import json
    from vit_prisma_amd.model_loader import MODEL_ARCH, load_config
    with open(os.path.join(os.path.dirname(__file__), "golden", "model_registry.json")) as f:
        reg = json.load(f)
    assert sorted(reg) == sorted(MODEL_ARCH)
    for name, fields in reg.items():
        cfg = load_config(name, device="cpu")
        for k, v in fields.items():
            if k == "architecture":                       # (a loader-internal tag of the reference, not a HookedViTConfig field)
                continue
            assert getattr(cfg, k) == v, (name, k, getattr(cfg, k), v)
    a, b = load_config("openai/clip-vit-base-patch32", device="cpu"), load_config("open-clip:laion/CLIP-ViT-B-32-DataComp.XL-s13B-b90K", device="cpu")
    assert (a.eps, a.normalize_output) == (1e-6, False) and (b.eps, b.normalize_output) == (1e-5, True)


def test_sae_runner_config_contract_vs_reference_fixture():
    """VisionModelSAERunnerConfig against the reference's own class (tests/golden/sae_config_contract.json, generated by instantiating the
    reference's config: gen_golden_sae_config_contract.py): for six keyword sets every dataclass field after __post_init__, every
    property (device, dtype, hook_point, out_hook_point, tokens_per_buffer, total_training_*) and what assigning through the setters
    leaves behind -- e.g. ``cfg.hook_point = ...`` changes nothing (sae/config.py:428-436).  The one deliberate superset: _dtype =
    "bfloat16" resolves here and raises KeyError in the reference (its dtype table has no bf16 entry)."""
    import json
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    from gen_golden_sae_config_contract import contract
    from vit_prisma_amd.sae import VisionModelSAERunnerConfig
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sae_config_contract.json")) as f:
        G = json.load(f)
    mine = contract(VisionModelSAERunnerConfig)
    assert sorted(mine) == sorted(G)
    for tag in G:
        for sect in ("fields", "props", "after_setters"):
            assert sorted(mine[tag][sect]) == sorted(G[tag][sect]), (tag, sect)
            for k, want in G[tag][sect].items():
                if tag == "gated_bf16" and k == "dtype" and sect == "props":
                    assert want == "raises KeyError" and mine[tag][sect][k] == "torch.bfloat16"
                    continue
                assert mine[tag][sect][k] == want, (tag, sect, k, mine[tag][sect][k], want)


def test_hooked_vit_config_contract_vs_reference_fixture():
    """HookedViTConfig against the reference's own class (tests/golden/vit_config_contract.json: every one of its 89 dataclass fields after
    __post_init__ for the defaults, the two target architectures and the tiny test architecture; gen_golden_vit_config_contract.py)."""
    import json
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    from gen_golden_vit_config_contract import contract
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vit_config_contract.json")) as f:
        G = json.load(f)
    mine = contract(HookedViTConfig)
    assert mine == G


def test_fold_value_biases_vs_reference_fixture():
    """HookedViT.fold_value_biases / load_and_process_state_dict (base_vit.py:498-532, base_transformer.py:35-104; the reference's loader
    applies the folding BY DEFAULT) against the reference's own run on the tiny model (tests/golden/vit_tiny_fold_value_biases.npz): the
    b_O / b_V it leaves, and the output / cache of the folded model -- hook_v changes, the output does not."""
    from vit_prisma_amd.synth import ARCHS, synth_images, synth_vit_state
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vit_tiny_fold_value_biases.npz"))
    arch = ARCHS["tiny"]
    model = HookedViT(HookedViTConfig(**arch, dtype=torch.float32, device="cpu")).eval()
    sd = {k: torch.from_numpy(v.copy()) for k, v in synth_vit_state(arch, 0).items()}
    plain = HookedViT(HookedViTConfig(**arch, dtype=torch.float32, device="cpu")).eval()
    plain.load_state_dict(sd, strict=True)
    model.load_and_process_state_dict(dict(sd), fold_ln=False, center_writing_weights=False, fold_value_biases=True)
    for k in G.files:
        if k.startswith("param::"):
            got = model.state_dict()[k.split("::", 1)[1]].numpy()
            assert np.allclose(got, G[k], rtol=1e-6, atol=1e-7), k
    assert float(model.blocks[0].attn.b_V.abs().max()) == 0.0
    x = torch.from_numpy(synth_images(arch, 2, 1))
    with torch.no_grad():
        out, cache = model.run_with_cache(x)
        out_plain, cache_plain = plain.run_with_cache(x)
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))      # noqa: E731
    assert rel(out.numpy(), G["out"]) < 1e-5 and rel(out.numpy(), out_plain.numpy()) < 1e-5
    for k in G.files:
        if k.startswith("cache::"):
            assert rel(cache[k.split("::", 1)[1]].numpy(), G[k]) < 1e-5, k
    assert rel(cache["blocks.0.attn.hook_v"].numpy(), cache_plain["blocks.0.attn.hook_v"].numpy()) > 1e-3      # (the folding is visible in the cache)
    # the reference's own defaults (fold_ln = center_writing_weights = True): accepted, the two unbuilt rewrites skipped with a warning
    again = HookedViT(HookedViTConfig(**arch, dtype=torch.float32, device="cpu")).eval()
    again.load_and_process_state_dict(dict(sd))
    assert all(torch.equal(a, b) for a, b in zip(again.state_dict().values(), model.state_dict().values()))
    with pytest.raises(NotImplementedError):
        model.load_and_process_state_dict(dict(sd), refactor_factored_attn_matrices=True)


def test_construction_helpers_of_the_reference_surface(tmp_path):
    """HookedViT.from_local (a reference-trainer checkpoint: {"model_state_dict": ...}, base_vit.py:652-668), from_pretrained (the legacy
    entry point forwarding to load_hooked_model, base_transformer.py:320-364 -- offline: a local checkpoint or pretrained=False),
    move_model_modules_to_device."""
    from vit_prisma_amd.synth import ARCHS, synth_vit_state
    arch = ARCHS["tiny"]
    cfg = HookedViTConfig(**arch, dtype=torch.float32, device="cpu")
    src = HookedViT(cfg).eval()
    src.load_state_dict({k: torch.from_numpy(v) for k, v in synth_vit_state(arch, 0).items()}, strict=True)
    path = os.path.join(tmp_path, "ckpt.pt")
    torch.save({"model_state_dict": src.state_dict(), "epoch": 3}, path)
    model = HookedViT.from_local(cfg, path)
    assert all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), src.state_dict().values()))
    with pytest.raises(Exception, match="no file was found"):
        HookedViT.from_local(cfg, os.path.join(tmp_path, "missing.pt"))
    assert model.move_model_modules_to_device() is model
    rnd = HookedViT.from_pretrained("openai/clip-vit-base-patch32", fold_ln=False, center_writing_weights=False, device="cpu", pretrained=False)
    assert type(rnd) is HookedViT and rnd.cfg.n_layers == 12 and rnd.cfg.eps == 1e-6
    legacy = HookedViT.from_pretrained("openai/clip-vit-base-patch32", device="cpu", pretrained=False)      # (the reference's own defaults work)
    assert type(legacy) is HookedViT and legacy.cfg.n_layers == 12
    with pytest.raises(NotImplementedError):
        HookedViT.from_pretrained("openai/clip-vit-base-patch32", device="cpu", pretrained=False, refactor_factored_attn_matrices=True)
