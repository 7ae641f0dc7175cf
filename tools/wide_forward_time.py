"""First timings of a wide-head tower on the HIP plan (HIP events, one JSON line): images/s of the all-hooks run_with_cache of
``load_hooked_model(name, pretrained=False)`` in bf16 at batch 32, beside the same call under use_native(False) -- what such a model ran
before attn_wide_kernel -- and their ratio; us per layer of the attention launch from the library's own profiler.  The socket's power
and clocks (rocm-smi, read only) are noted before and after.

    python tools/wide_forward_time.py [--model h14|g14|bigg14|l14-224] [--batch 32] [--steps 20] [--warmup 3] [--no-baseline]

``l14-224`` is CLIP L/14 at 224 px (T = 257, d_head 64: attn_lean_kernel), for context.  Under ``rocprofv3 --kernel-trace --stats`` use a
few steps and --no-baseline: the per-kernel times come from the trace."""
import argparse, json, os, subprocess, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vit_prisma_amd import HookedViT, _native as N
from vit_prisma_amd.model_loader import load_config, load_hooked_model

NAMES = {"h14": "open-clip:laion/CLIP-ViT-H-14-laion2B-s32B-b79K", "g14": "open-clip:laion/CLIP-ViT-g-14-laion2B-s34B-b88K",
         "bigg14": "open-clip:laion/CLIP-ViT-bigG-14-laion2B-39B-b160k"}
ap = argparse.ArgumentParser()
ap.add_argument("--model", default="h14", choices=sorted(NAMES) + ["l14-224"])
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--no-baseline", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda:0")


def socket_state():
    try:
        r = subprocess.run(["rocm-smi", "-d", "0", "--showpower", "--showclocks", "--showperflevel"], capture_output=True, text=True, timeout=60)
        keep = [ln.strip() for ln in r.stdout.splitlines() if any(w in ln for w in ("Power", "sclk", "mclk", "Performance Level"))]
        return keep
    except Exception as e:                                                     # noqa: BLE001
        return [f"rocm-smi unavailable: {e}"]


def images_per_s(model, images, steps, warmup):
    for _ in range(warmup):
        o, c = model.run_with_cache(images); del o, c
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        o, c = model.run_with_cache(images); del o, c
    e1.record(); torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    return round(images.shape[0] / ms * 1e3, 1), round(ms, 2)


out = {"model": args.model, "batch": args.batch, "steps": args.steps, "warmup": args.warmup, "socket_before": socket_state()}
torch.manual_seed(0)
with torch.no_grad():
    if args.model == "l14-224":
        cfg = load_config("openai/clip-vit-large-patch14-336", dtype=torch.bfloat16, device="cuda", image_size=224)
        model = HookedViT(cfg).to(torch.bfloat16).to(dev).eval()
    else:
        model = load_hooked_model(NAMES[args.model], pretrained=False, dtype=torch.bfloat16, device="cuda").eval()
    out.update(n_layers=model.cfg.n_layers, d_head=model.cfg.d_head, n_tokens=model.n_tokens)
    images = torch.randn(args.batch, 3, 224, 224, device=dev, generator=torch.Generator(device=dev).manual_seed(1)).bfloat16()
    out["native_images_per_s"], out["native_ms_per_step"] = images_per_s(model.use_native(True), images, args.steps, args.warmup)
    assert model.last_run_native, model.native_fallback_reason
    N.prof_reset(); N.prof_enable(True, kinds=("attention",))
    for _ in range(3):
        o, c = model.run_with_cache(images); del o, c
    torch.cuda.synchronize(); N.prof_enable(False)
    r = N.prof_read("attention")
    out["attention_us_per_layer_all_hooks"] = round(r["ms"] / r["launches"] * 1e3, 1)
    if not args.no_baseline:
        out["pytorch_images_per_s"], out["pytorch_ms_per_step"] = images_per_s(model.use_native(False), images, args.steps, args.warmup)
        assert not model.last_run_native
        out["ratio"] = round(out["native_images_per_s"] / out["pytorch_images_per_s"], 2)
out["socket_after"] = socket_state()
print(json.dumps(out))
