"""Fixtures of the text tower (HookedTextTransformer), produced from the reference on the CPU (build container only):

    python tests/golden/gen_golden_text.py   ->  tests/golden/text_tiny_full.npz
                                                 tests/golden/text_tiny_bf16_budget.json
                                                 tests/golden/weight_conversion_text_tiny.npz
                                                 tests/golden/model_registry_text.json

* text_tiny_full.npz: the reference's HookedTextTransformer (fp32) on ``synth.ARCHS["tiny-text"]`` (2 layers, d_model 128, 2 heads of
  64, context 77, vocab 96) from ``synth_text_state`` seed 0 on ``synth_tokens`` (batch 2: row 0 ends in the EOT, row 1 has it at 40
  AND 55): the key order (``__keys__``), the output (``__out__``), the ids (``__tokens__``) and ``__parts__``; every cache tensor of
  the fp32 run in text_tiny_full.part{i}.npz, in firing order (parts: no committed file above 1 MiB; tests/_text_fixture.py reads
  them back as one mapping).
* text_tiny_bf16_budget.json: per key, the rel-Frobenius error of the reference's OWN bf16 run (cfg.dtype = bfloat16, .to(bfloat16))
  against its fp32 run over the positions that are finite in the fp32 run, and the key's dtype in the bf16 run; ``__out__`` too.
* weight_conversion_text_tiny.npz: a random open_clip-format text state dict (``in.*``; d_model 64, 2 heads of 32, ``__cfg__``) and
  what the reference's convert_open_clip_text_weights makes of it (``out.*``, key order ``__out_keys__``).
* model_registry_text.json: the fields of OPEN_CLIP_TEXT_CONFIGS (models/model_config_registry.py:605-674) as data, read like
  gen_golden_vit_wide.py reads the registry."""
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
import _refimport  # noqa: E402
from vit_prisma_amd.synth import ARCHS, synth_text_state, synth_tokens  # noqa: E402

BATCH = 2
_refimport.install()
from vit_prisma.configs.HookedTextTransformerConfig import HookedTextTransformerConfig  # noqa: E402
from vit_prisma.models.base_text_transformer import HookedTextTransformer  # noqa: E402
from vit_prisma.models.weight_conversion import convert_open_clip_text_weights  # noqa: E402

arch = ARCHS["tiny-text"]
tokens = torch.from_numpy(synth_tokens(arch, BATCH, seed=1))
sd = {k: torch.from_numpy(v) for k, v in synth_text_state(arch, seed=0).items()}


def run(dtype):
    model = HookedTextTransformer(HookedTextTransformerConfig(**arch, dtype=dtype, device="cpu"))
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert sorted(missing) == ["ln_pre.b", "ln_pre.w"] and not unexpected, (missing, unexpected)
    model = model.to(dtype).eval()
    with torch.no_grad():
        out, cache = model.run_with_cache(tokens)
    return out, cache.cache_dict


out32, c32 = run(torch.float32)
# the tensors go into parts of at most PART_BYTES each (no committed file above 1 MiB), in firing order; text_tiny_full.npz itself
# holds the key order, the output, the ids and the number of parts (tests/_text_fixture.py puts them together again)
PART_BYTES = 900 * 1024
parts, cur, size = [], {}, 0
for k, v in c32.items():
    a = np.ascontiguousarray(v.numpy())
    if cur and size + a.nbytes > PART_BYTES:
        parts.append(cur)
        cur, size = {}, 0
    cur[k] = a
    size += a.nbytes
parts.append(cur)
for stale in [f for f in os.listdir(HERE) if f.startswith("text_tiny_full.part")]:
    os.remove(os.path.join(HERE, stale))
for i, part in enumerate(parts):
    path = os.path.join(HERE, f"text_tiny_full.part{i}.npz")
    np.savez_compressed(path, **part)
    print(os.path.basename(path), len(part), "keys", os.path.getsize(path) // 1024, "kB")
np.savez_compressed(os.path.join(HERE, "text_tiny_full.npz"), __out__=out32.numpy(), __keys__=np.array(list(c32.keys())),
                    __tokens__=tokens.numpy(), __parts__=np.int64(len(parts)))
print(list(c32.keys()))

out16, c16 = run(torch.bfloat16)
assert list(c16.keys()) == list(c32.keys())


def rel(a16, a32):
    a, b = a16.double(), a32.double()
    fin = torch.isfinite(b)
    assert torch.equal(torch.isinf(a), torch.isinf(b)), "the bf16 run's -inf positions differ from the fp32 run's"
    return float((a[fin] - b[fin]).norm() / b[fin].norm().clamp_min(1e-30))


budget = {k: {"rel_fro": rel(c16[k], c32[k]), "dtype": str(c16[k].dtype).replace("torch.", "")} for k in c32}
budget["__out__"] = {"rel_fro": rel(out16, out32), "dtype": str(out16.dtype).replace("torch.", "")}
with open(os.path.join(HERE, "text_tiny_bf16_budget.json"), "w") as f:
    json.dump(budget, f, indent=1)
print("bf16 out rel", budget["__out__"])

# ---- converter (a smaller shape than the tower above: the file holds the state dict twice)
CONV_ARCH = dict(arch, d_model=64, n_heads=2, d_head=32, d_mlp=128, vocab_size=40, n_classes=24)
arch = CONV_ARCH
cfg = HookedTextTransformerConfig(**arch, dtype=torch.float32, device="cpu")
rs = np.random.RandomState(7)
d, dm, L = arch["d_model"], arch["d_mlp"], arch["n_layers"]


def nrm(*shape):
    return torch.from_numpy(rs.standard_normal(size=shape).astype(np.float32))


old = {"token_embedding.weight": nrm(arch["vocab_size"], d), "positional_embedding": nrm(arch["context_length"], d),
       "ln_final.weight": nrm(d), "ln_final.bias": nrm(d), "text_projection": nrm(d, arch["n_classes"])}
for l in range(L):
    p = f"transformer.resblocks.{l}"
    old.update({p + ".attn.in_proj_weight": nrm(3 * d, d), p + ".attn.in_proj_bias": nrm(3 * d),
                p + ".attn.out_proj.weight": nrm(d, d), p + ".attn.out_proj.bias": nrm(d),
                p + ".ln_1.weight": nrm(d), p + ".ln_1.bias": nrm(d), p + ".ln_2.weight": nrm(d), p + ".ln_2.bias": nrm(d),
                p + ".mlp.c_fc.weight": nrm(dm, d), p + ".mlp.c_fc.bias": nrm(dm),
                p + ".mlp.c_proj.weight": nrm(d, dm), p + ".mlp.c_proj.bias": nrm(d)})
new = convert_open_clip_text_weights(old, cfg)
conv = {"in." + k: v.numpy() for k, v in old.items()}
conv.update({"out." + k: np.ascontiguousarray(v.numpy()) for k, v in new.items()})
conv["__out_keys__"] = np.array(list(new.keys()))
conv["__cfg__"] = np.array(json.dumps({k: arch[k] for k in ("n_layers", "d_model", "n_heads", "d_head", "d_mlp", "vocab_size", "context_length", "n_classes")}))
path = os.path.join(HERE, "weight_conversion_text_tiny.npz")
np.savez_compressed(path, **conv)
print("weight_conversion_text_tiny.npz", len(new), "keys", os.path.getsize(path) // 1024, "kB")

# ---- registry
REG = os.path.join(_refimport.REF_SRC, "vit_prisma", "models", "model_config_registry.py")
stub = types.ModuleType("vit_prisma.utils.enums")


class _ModelType:                                     # the registry only uses it as dict keys further down
    VISION = "VISION"
    TEXT = "TEXT"


stub.ModelType = _ModelType
sys.modules["vit_prisma.utils.enums"] = stub
ns = {"__name__": "registry"}
with open(REG) as f:
    exec(compile(f.read(), REG, "exec"), ns)
table = ns["OPEN_CLIP_TEXT_CONFIGS"]
reg = {name: {k: v for k, v in entry.items() if isinstance(v, (int, float, str, bool))} for name, entry in sorted(table.items())}
print(len(reg), "text names")
with open(os.path.join(HERE, "model_registry_text.json"), "w") as f:
    json.dump(reg, f, indent=1, sort_keys=True)
