"""Fixtures of the DINO family, produced by executing the reference on the CPU (build container only):

    python tests/golden/gen_golden_dino.py   ->  tests/golden/vit_tiny_pooled_heads.npz
                                                 tests/golden/weight_conversion_dino_tiny.npz
                                                 tests/golden/model_registry_dino.json

* vit_tiny_pooled_heads.npz: the reference's HookedViT (fp32) on two tiny models from seeded synthetic weights (seed 5; the arch
  tables are tests/test_dino_cpu.py's POOLED_ARCHS) -- ``classification_type="gaap"`` and the name ``facebook/dino-vitb-tiny`` with
  ``return_type="pre_logits"`` (base_vit.py:195-208) -- batch 3: output, key order, hook_ln_final, hook_post_head_pre_normalize.
* weight_conversion_dino_tiny.npz: a seeded synthetic HuggingFace ``ViTModel`` checkpoint (test_dino_cpu.synth_hf_vit_state, seed 4)
  and what the reference's ``convert_dino_weights`` (models/weight_conversion.py:432-518) returned for it.
* model_registry_dino.json: the four DINO entries of the reference's registry (models/model_config_registry.py:544-570), as data --
  read like gen_golden_model_registry.py does, without importing the package."""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
from _refimport import REF_SRC, install, reference_classes  # noqa: E402
from test_dino_cpu import POOLED_ARCHS, POOLED_BATCH, POOLED_KEYS, dino_tiny_cfg, synth_hf_vit_state  # noqa: E402
from vit_prisma_amd.synth import synth_images, synth_vit_state  # noqa: E402

install()
from vit_prisma.models.weight_conversion import convert_dino_weights as ref_dino  # noqa: E402

# ---- pooled heads
R = reference_classes()
blob = {}
for tag, arch in POOLED_ARCHS.items():
    model = R["HookedViT"](R["HookedViTConfig"](**arch, dtype=torch.float32, device="cpu"))
    own = model.state_dict()
    sd = {k: torch.from_numpy(v) for k, v in synth_vit_state(arch, seed=5).items() if k in own}
    missing, unexpected = model.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    model.eval()
    with torch.no_grad():
        out, cache = model.run_with_cache(torch.from_numpy(synth_images(arch, POOLED_BATCH, 1)))
    blob[f"{tag}::__out__"] = out.numpy()
    blob[f"{tag}::__keys__"] = np.array(list(cache.cache_dict.keys()))
    for k in POOLED_KEYS:
        blob[f"{tag}::{k}"] = np.ascontiguousarray(cache.cache_dict[k].numpy())
    print(tag, tuple(out.shape), [(k, blob[f"{tag}::{k}"].shape) for k in POOLED_KEYS])
path = os.path.join(HERE, "vit_tiny_pooled_heads.npz")
np.savez_compressed(path, **blob)
print(os.path.getsize(path) // 1024, "kB")

# ---- converter
cfg = dino_tiny_cfg()
sd = synth_hf_vit_state(cfg, seed=4)
blob = {}
for prefix, d in (("in_hf", sd), ("ref", ref_dino(sd, cfg))):
    for k, v in d.items():
        blob[f"{prefix}::{k}"] = v.detach().cpu().numpy().copy()
path = os.path.join(HERE, "weight_conversion_dino_tiny.npz")
np.savez_compressed(path, **blob)
print(len(blob), "arrays,", os.path.getsize(path) // 1024, "kB")

# ---- registry
REG = os.path.join(REF_SRC, "vit_prisma", "models", "model_config_registry.py")
stub = types.ModuleType("vit_prisma.utils.enums")


class _ModelType:                                     # the registry only uses it as dict keys further down
    VISION = "VISION"
    TEXT = "TEXT"


stub.ModelType = _ModelType
sys.modules["vit_prisma.utils.enums"] = stub
ns = {"__name__": "registry"}
with open(REG) as f:
    exec(compile(f.read(), REG, "exec"), ns)
out = {name: {k: v for k, v in entry.items() if isinstance(v, (int, float, str, bool))} for name, entry in sorted(ns["DINO_CONFIGS"].items())}
for name, entry in out.items():
    print(name, entry)
with open(os.path.join(HERE, "model_registry_dino.json"), "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
