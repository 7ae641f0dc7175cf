"""Golden outputs of the reference's patch-level logit lens on the tiny model (build container only): executes
/root/reference's prisma_tools/logit_lens.py on a cache produced by the reference HookedViT, with all_answers = head.W_H.T,
both incl_mid values and a rank label.  The dictionary goes into the npz as arrays [T, S]: logits, class indices, ranks."""
import os, sys
import numpy as np, torch
HERE = os.path.dirname(os.path.abspath(__file__)); ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, HERE)
from gen_golden_vit import build_reference_model, run_ref
from vit_prisma_amd.synth import synth_images

RANK_INDEX = 5
BATCH_IDX = 1

model, arch = build_reference_model("tiny")          # (installs the reference import shells)
from vit_prisma.prisma_tools.logit_lens import get_patch_logit_directions, get_patch_logit_dictionary  # noqa: E402
from vit_prisma.utils.data_utils.imagenet.imagenet_dict import IMAGENET_DICT  # noqa: E402
from vit_prisma.utils.data_utils.imagenet.imagenet_utils import imagenet_index_from_word  # noqa: E402
out, cache = run_ref(model, synth_images(arch, 2, 1))
answers = model.head.W_H.detach().T.contiguous()
rank_label = IMAGENET_DICT[RANK_INDEX]
assert imagenet_index_from_word(rank_label) == RANK_INDEX
blob = {"rank_index": np.array(RANK_INDEX), "batch_idx": np.array(BATCH_IDX), "answers": answers.numpy()}
for incl_mid in (False, True):
    tag = "mid" if incl_mid else "pre"
    directions, labels = get_patch_logit_directions(cache, answers, incl_mid=incl_mid)
    blob[f"directions_{tag}"] = np.ascontiguousarray(directions.numpy())
    blob[f"labels_{tag}"] = np.array(labels)
    table = get_patch_logit_dictionary((directions, labels), batch_idx=BATCH_IDX, rank_label=rank_label)
    T, S = directions.shape[1], directions.shape[2]
    assert sorted(table) == list(range(T)) and all(len(table[t]) == S for t in table)
    blob[f"dict_logit_{tag}"] = np.array([[table[t][s][0] for s in range(S)] for t in range(T)], dtype=np.float32)
    blob[f"dict_index_{tag}"] = np.array([[table[t][s][2] for s in range(S)] for t in range(T)], dtype=np.int64)
    blob[f"dict_rank_{tag}"] = np.array([[int(table[t][s][3]) for s in range(S)] for t in range(T)], dtype=np.int64)
    plain = get_patch_logit_dictionary(directions, batch_idx=BATCH_IDX)
    assert all(len(cell) == 3 for t in plain for cell in plain[t])
np.savez_compressed(os.path.join(HERE, "logit_lens_tiny.npz"), **blob)
print({k: v.shape for k, v in blob.items()})
