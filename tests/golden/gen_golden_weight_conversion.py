"""The reference's weight converters (models/weight_conversion.py: convert_open_clip_weights, and convert_kandinsky_clip_weights, its
HuggingFace CLIPModel converter) on the tiny model's seeded synthetic open_clip checkpoint (seed 3) and on the same weights under
HuggingFace names (build container only): the checkpoint and what the reference returned for each form.

    python tests/golden/gen_golden_weight_conversion.py     ->  tests/golden/weight_conversion_tiny.npz"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
from _refimport import install  # noqa: E402
from test_weights_transforms_cpu import synth_open_clip_state, tiny_cfg, to_hf_names  # noqa: E402

install()
from vit_prisma.models.weight_conversion import convert_kandinsky_clip_weights as ref_hf  # noqa: E402
from vit_prisma.models.weight_conversion import convert_open_clip_weights as ref_oc  # noqa: E402

cfg = tiny_cfg()
sd = synth_open_clip_state(cfg, seed=3)
hf_sd = to_hf_names(sd, cfg)
blob = {}
for prefix, d in (("in_open_clip", sd), ("ref_open_clip", ref_oc(sd, cfg)),
                  ("ref_hf", ref_hf(hf_sd, cfg, device="cpu"))):
    for k, v in d.items():
        blob[f"{prefix}::{k}"] = v.detach().cpu().numpy().copy()
out = os.path.join(HERE, "weight_conversion_tiny.npz")
np.savez_compressed(out, **blob)
print(len(blob), "arrays,", os.path.getsize(out) // 1024, "kB")
