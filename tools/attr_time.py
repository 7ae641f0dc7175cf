"""HIP-event times and peak memory of the direct logit attribution by head (vit_prisma_amd/logit_attribution.py) on a CLIP ViT-B/32 in
bf16, one JSON line per form: the HIP path beside the PyTorch path of the same call (``use_native(False)``: the reference's
composition one layer at a time) and beside the reference's helpers themselves (``stack_head_results(apply_ln=True)`` and an einsum:
the whole [L H, B, T, d_model] stack), in the same process.

    python tools/attr_time.py [--images 512] [--answers 1] [--steps 10] [--torch-steps 2] [--warmup 2] [--rounds 2] [--no-helpers]
    python tools/attr_time.py --neurons [--images 512] [--steps 10] [--torch-steps 1] [--rounds 2]      # by MLP neuron (below)

Forms: shared answers [O, d] and per-image answers [B, O, d], each with pos=None (every token) and pos=0 (the CLS row).  Every form
is warmed up before it is timed, a timed window is ``steps`` calls between two events, and the set is repeated ``rounds`` times in
alternation.  Bytes per call: the hook_z taps once (B T L H d_head 2; with a pos, one row in T of them) plus the output
(B T_out L H O 4); the fold's operands (W_O: L H d_head d 2, the answers) stand beside them as ``fold_mbytes``.  Peak memory is
``torch.cuda.max_memory_allocated`` over one call minus what was allocated before it (the cache and the model are not counted)."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vit_prisma_amd import HookedViT, HookedViTConfig, logit_attribution
from vit_prisma_amd.logit_attribution import head_logit_attribution
from vit_prisma_amd.synth import ARCHS, synth_vit_state

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=512)
ap.add_argument("--answers", type=int, default=1)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--torch-steps", type=int, default=2)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--no-helpers", action="store_true", help="skip the reference helpers' own composition (the full stack)")
ap.add_argument("--neurons", action="store_true", help="time the attribution by MLP neuron (dense with pos=0, top-k over every token) instead")
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


def peak_mbytes(fn):
    """MB allocated at the peak of one call beyond what was allocated before it"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return round(peak / 1e6, 1)


arch = ARCHS["clip-vit-b32"]
model = HookedViT(HookedViTConfig(**arch, dtype=torch.bfloat16, device="cuda"))
model.load_state_dict({k: torch.from_numpy(v) for k, v in synth_vit_state(arch, 0).items()}, strict=True)
model = model.to(torch.bfloat16).to(dev).eval().use_native(True)
d, L, H, dh = arch["d_model"], arch["n_layers"], arch["n_heads"], arch["d_head"]
B, O = args.images, args.answers

with torch.no_grad():
    images = torch.randn(B, 3, arch["image_size"], arch["image_size"], device=dev,
                         generator=torch.Generator(device=dev).manual_seed(1)).bfloat16()
    _, cache = model.run_with_cache(images)
    assert model.last_run_native, model.native_fallback_reason
    del images
    T = cache["ln_final.hook_scale"].shape[1]
    gen = torch.Generator(device=dev).manual_seed(2)
    answers = {"shared": 0.05 * torch.randn(O, d, device=dev, generator=gen) + 0.02,
               "per_image": 0.05 * torch.randn(B, O, d, device=dev, generator=gen) + 0.02}

    def helpers(a, pos):
        """the reference's three steps: compute_head_results (cached by the helper; dropped again here), the stack, the product"""
        stack = cache.stack_head_results(-1, apply_ln=True, pos_slice=None if pos is None else [pos])
        for l in range(L):
            del cache.cache_dict[f"blocks.{l}.attn.hook_result"]
        eq = "cbtd,bod->cbto" if a.dim() == 3 else "cbtd,od->cbto"
        return torch.einsum(eq, stack, a).permute(1, 2, 0, 3)

    def neuron_forms():
        """--neurons: the dense form with pos=0 and one answer per image, the top-k form (k = 16) over every token with O = 1 and with
        O = 4 shared answers; each beside the PyTorch path of the same call on the same cache.  Bytes: the mlp.hook_post taps once
        (B T_out L d_mlp 2); the fold's operands (W_out, the answers) and G (L R d_mlp 4, read by every workgroup from the L2)
        stand beside them."""
        M = arch["d_mlp"]
        a4 = 0.05 * torch.randn(4, d, device=dev, generator=gen) + 0.02
        forms = [("dense", answers["per_image"][:, :1].contiguous(), 0, None), ("topk", answers["shared"][:1].contiguous(), None, 16),
                 ("topk", a4, None, 16)]
        for form, a, pos, k in forms:
            t_out = T if pos is None else 1
            n_ans = a.shape[-2]
            tap_bytes = B * t_out * L * M * 2
            out_bytes = B * t_out * L * M * n_ans * 4 if k is None else B * t_out * n_ans * k * 8
            row = {"form": form, "images": B, "tokens": T, "layers": L, "d_mlp": M, "d_model": d, "answers": n_ans,
                   "kind": "per_image" if a.dim() == 3 else "shared", "pos": pos, "k": k, "tap_mbytes": round(tap_bytes / 1e6, 1),
                   "out_mbytes": round(out_bytes / 1e6, 2), "fold_mbytes": round((L * M * d * 2 + a.numel() * 4) / 1e6, 1),
                   "g_mbytes": round(L * M * a.numel() / d * 4 / 1e6, 2),
                   "gflop": round((2.0 * B * t_out * L * M * n_ans + 2.0 * L * M * d * a.numel() / d) / 1e9, 2)}
            if k is None:
                fn = lambda: logit_attribution.neuron_logit_attribution(cache, a, pos=pos, return_labels=False)      # noqa: E731
            else:
                fn = lambda: logit_attribution.top_neuron_logit_attribution(cache, a, k, pos=pos, by="abs")          # noqa: E731
            native_ms, torch_ms = [], []
            for _ in range(args.rounds):
                logit_attribution.use_native(True)
                native_ms.append(round(timed(fn, args.steps, args.warmup), 4))
                assert logit_attribution.last_run_native
            logit_attribution.use_native(True)
            row["native_peak_mbytes"] = peak_mbytes(fn)
            best = min(native_ms)
            row.update(native_ms=native_ms, native_read_gbytes_per_s=round(tap_bytes / 1e6 / best, 1),
                       native_gbytes_per_s=round((tap_bytes + out_bytes) / 1e6 / best, 1))
            logit_attribution.use_native(False)
            try:
                for _ in range(args.torch_steps):               # (--torch-steps 0: the HIP path alone, for a kernel trace)
                    torch_ms.append(round(timed(fn, 1, 0), 2))
                    assert not logit_attribution.last_run_native
                if torch_ms:
                    row["pytorch_peak_mbytes"] = peak_mbytes(fn)
                    row.update(pytorch_ms=torch_ms, pytorch_over_native=round(min(torch_ms) / best, 1))
            except torch.cuda.OutOfMemoryError:
                row["pytorch_ms"] = "out of memory at this shape"
                torch.cuda.empty_cache()
            logit_attribution.use_native(None)
            print(json.dumps(row), flush=True)

    if args.neurons:
        neuron_forms()
        sys.exit(0)

    for kind, a in answers.items():
        for pos in (None, 0):
            t_out = T if pos is None else 1
            tap_bytes = B * t_out * L * H * dh * 2
            out_bytes = B * t_out * L * H * O * 4
            row = {"images": B, "tokens": T, "layers": L, "heads": H, "d_head": dh, "d_model": d, "answers": O, "kind": kind,
                   "pos": pos, "tap_mbytes": round(tap_bytes / 1e6, 1), "out_mbytes": round(out_bytes / 1e6, 2),
                   "fold_mbytes": round((L * H * dh * d * 2 + a.numel() * 4) / 1e6, 1),
                   "gflop": round((2.0 * B * t_out * L * H * dh * O + 2.0 * L * H * dh * d * a.numel() / d) / 1e9, 2)}
            fn = lambda: head_logit_attribution(cache, a, pos=pos, return_labels=False)      # noqa: E731
            native_ms, torch_ms = [], []
            for _ in range(args.rounds):
                logit_attribution.use_native(True)
                native_ms.append(round(timed(fn, args.steps, args.warmup), 4))
                assert logit_attribution.last_run_native
                logit_attribution.use_native(False)
                torch_ms.append(round(timed(fn, args.torch_steps, 1), 4))
                assert not logit_attribution.last_run_native
            logit_attribution.use_native(True)
            row["native_peak_mbytes"] = peak_mbytes(fn)
            logit_attribution.use_native(False)
            row["pytorch_peak_mbytes"] = peak_mbytes(fn)
            logit_attribution.use_native(None)
            best = min(native_ms)
            row.update(native_ms=native_ms, pytorch_ms=torch_ms, pytorch_over_native=round(min(torch_ms) / best, 1),
                       native_read_gbytes_per_s=round(tap_bytes / 1e6 / best, 1),
                       native_gbytes_per_s=round((tap_bytes + out_bytes) / 1e6 / best, 1))
            if not args.no_helpers:
                try:
                    row["helpers_ms"] = round(timed(lambda: helpers(a, pos), 1, 1), 3)
                    row["helpers_peak_mbytes"] = peak_mbytes(lambda: helpers(a, pos))
                except torch.cuda.OutOfMemoryError:
                    row["helpers_ms"] = "out of memory at this shape"
                    for l in range(L):
                        cache.cache_dict.pop(f"blocks.{l}.attn.hook_result", None)
                    torch.cuda.empty_cache()
            print(json.dumps(row), flush=True)
