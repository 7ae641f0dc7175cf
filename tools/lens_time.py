"""HIP-event times of the patch-level logit lens (vit_prisma_amd/logit_lens.py) on a CLIP ViT-B/32 in bf16, one JSON line per shape:
the directions form and the top form on the HIP path, beside the PyTorch path of the same functions (``use_native(False)``) in the
same process, and the all-hooks forward that produced the cache, for scale.

    python tools/lens_time.py [--images 512 1] [--answers 512 1000] [--steps 10] [--torch-steps 3] [--warmup 2] [--rounds 2]

Shapes: 512 images (N = 25 600 rows per tap) and 1 image (N = 50), S = 13 (incl_mid=False) and 25, O = 512 and 1000.  Every form is
warmed up on its shape before it is timed, a timed window is ``steps`` calls between two events, and the whole set is repeated
``rounds`` times in alternation (native, PyTorch, native, ...) so that the spread between rounds stands beside the ratio.
Algorithmic work per call: 2 N S O d flops; bytes = the taps once (N S d 2) + the answers + the output (directions: N S O 4; top:
N S 12)."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vit_prisma_amd import HookedViT, HookedViTConfig, logit_lens
from vit_prisma_amd.synth import ARCHS, synth_vit_state

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, nargs="+", default=[512, 1])
ap.add_argument("--answers", type=int, nargs="+", default=[512, 1000])
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--torch-steps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--rounds", type=int, default=2)
args = ap.parse_args()
assert torch.cuda.is_available(), "this tool measures on the GPU; there is no CPU substitute for its numbers"
dev = torch.device("cuda:0")


def timed(fn, steps, warmup):
    """ms per call between two events on the current stream"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


arch = ARCHS["clip-vit-b32"]
model = HookedViT(HookedViTConfig(**arch, dtype=torch.bfloat16, device="cuda"))
model.load_state_dict({k: torch.from_numpy(v) for k, v in synth_vit_state(arch, 0).items()}, strict=True)
model = model.to(torch.bfloat16).to(dev).eval().use_native(True)
d = arch["d_model"]

with torch.no_grad():
    for n_img in args.images:
        images = torch.randn(n_img, 3, arch["image_size"], arch["image_size"], device=dev,
                             generator=torch.Generator(device=dev).manual_seed(1)).bfloat16()
        forward_ms = timed(lambda: model.run_with_cache(images), args.steps, args.warmup)
        assert model.last_run_native, model.native_fallback_reason
        _, cache = model.run_with_cache(images)
        N = n_img * cache["ln_final.hook_scale"].shape[1]
        for incl_mid in (False, True):
            for O in args.answers:
                answers = (0.05 * torch.randn(O, d, device=dev, generator=torch.Generator(device=dev).manual_seed(2))).bfloat16()
                forms = {
                    "directions": lambda: logit_lens.get_patch_logit_directions(cache, answers, incl_mid=incl_mid),
                    "top": lambda: logit_lens.patch_logit_top(cache, answers, incl_mid=incl_mid, rank_index=O // 2),
                }
                S = 2 * arch["n_layers"] + 1 if incl_mid else arch["n_layers"] + 1
                row = {"images": n_img, "rows_per_tap": N, "stack": S, "answers": O, "d_model": d, "forward_all_hooks_ms": round(forward_ms, 3),
                       "gflop": round(2.0 * N * S * O * d / 1e9, 2),
                       "mbytes": {"directions": round((N * S * d * 2 + O * d * 2 + N * S * O * 4) / 1e6, 1),
                                  "top": round((N * S * d * 2 + O * d * 2 + N * S * 12) / 1e6, 1)}}
                for name, fn in forms.items():
                    native_ms, torch_ms = [], []
                    for _ in range(args.rounds):
                        logit_lens.use_native(True)
                        native_ms.append(round(timed(fn, args.steps, args.warmup), 4))
                        assert logit_lens.last_run_native
                        logit_lens.use_native(False)
                        torch_ms.append(round(timed(fn, args.torch_steps, 1), 4))
                        assert not logit_lens.last_run_native
                    logit_lens.use_native(None)
                    best_n, best_t = min(native_ms), min(torch_ms)
                    row[name] = {"native_ms": native_ms, "pytorch_ms": torch_ms, "pytorch_over_native": round(best_t / best_n, 2),
                                 "native_tflops": round(row["gflop"] / best_n, 2), "native_gbytes_per_s": round(row["mbytes"][name] / best_n, 1),
                                 "native_over_forward": round(best_n / forward_ms, 3)}
                print(json.dumps(row), flush=True)
        del cache
        torch.cuda.empty_cache()
