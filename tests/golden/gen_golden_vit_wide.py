"""Fixtures of the wide-head CLIP towers (ViT-H/14, g/14, bigG/14: d_head 80, 88, 104), produced from the reference on the CPU
(build container only):

    python tests/golden/gen_golden_vit_wide.py   ->  tests/golden/vit_tiny_wide.npz
                                                     tests/golden/model_registry_wide.json

* vit_tiny_wide.npz: the reference's HookedViT (fp32) on ``synth.ARCHS["tiny-wide"]`` (2 layers, d_model 160, 2 heads of 80, T = 17)
  from ``synth_vit_state`` seed 0, batch 3 of ``synth_images``: every cache tensor, the key order and the output, like
  vit_tiny_full.npz (gen_golden_vit.py).
* model_registry_wide.json: the registry's override fields for the names of ``model_loader.WIDE_ARCH``
  (models/model_config_registry.py:253-258, 326-328), as data -- read like gen_golden_model_registry.py does, without importing the
  package."""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from _refimport import REF_SRC, reference_classes  # noqa: E402
from vit_prisma_amd.model_loader import WIDE_ARCH  # noqa: E402
from vit_prisma_amd.synth import ARCHS, synth_images, synth_vit_state  # noqa: E402

BATCH = 3

# ---- the tiny wide model
R = reference_classes()
arch = ARCHS["tiny-wide"]
model = R["HookedViT"](R["HookedViTConfig"](**arch, dtype=torch.float32, device="cpu"))
sd = {k: torch.from_numpy(v) for k, v in synth_vit_state(arch, seed=0).items()}
missing, unexpected = model.load_state_dict(sd, strict=True)
assert not missing and not unexpected
model.eval()
with torch.no_grad():
    out, cache = model.run_with_cache(torch.from_numpy(synth_images(arch, BATCH, seed=1)))
blob = {"__out__": out.numpy(), "__keys__": np.array(list(cache.cache_dict.keys()))}
for k, v in cache.cache_dict.items():
    blob[k] = np.ascontiguousarray(v.numpy())
path = os.path.join(HERE, "vit_tiny_wide.npz")
np.savez_compressed(path, **blob)
print("vit_tiny_wide.npz", len(cache.cache_dict), "keys", os.path.getsize(path) // 1024, "kB")

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
table = ns["OPEN_CLIP_CONFIGS"]
reg = {name: {k: v for k, v in table[name].items() if isinstance(v, (int, float, str, bool))} for name in sorted(WIDE_ARCH)}
for name, entry in reg.items():
    print(name, entry)
with open(os.path.join(HERE, "model_registry_wide.json"), "w") as f:
    json.dump(reg, f, indent=1, sort_keys=True)
