"""First timings of the DINO shapes on the HIP plan (HIP events, one JSON line):
  * ms per step of the all-hooks run_with_cache at bs = 32 -- dino-vitb8 (12 layers, T = 785, d_head 64) in bf16 and fp32, dino-vits8
    in bf16 -- beside the same call under use_native(False), and the ratio;
  * us per layer of the attention launch at that T with and without taps: attn_lean_kernel (bf16 / d_head 64) beside
    attn_stream_kernel on the same shape (tuning key attn_wg = 1), and attn_stream_kernel in fp32.
python tools/dino_forward_time.py [batch]"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vit_prisma_amd import HookedViT, _native as N
from vit_prisma_amd.model_loader import load_config

dev = torch.device("cuda:0")
bs = int(sys.argv[1]) if len(sys.argv) > 1 else 32


def ms_per_step(model, images, reps, **kw):
    for _ in range(2):
        o, c = model.run_with_cache(images, **kw); del o, c
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        o, c = model.run_with_cache(images, **kw); del o, c
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def attn_us_per_layer(model, images, **kw):
    N.prof_reset(); N.prof_enable(True, kinds=("attention",))
    for _ in range(3):
        o, c = model.run_with_cache(images, **kw); del o, c
    torch.cuda.synchronize(); N.prof_enable(False)
    r = N.prof_read("attention")
    return round(r["ms"] / r["launches"] * 1e3, 1)


out = {"batch": bs}
z_only = dict(names_filter=lambda n: n.endswith("attn.hook_z"))
with torch.no_grad():
    for name, dtype in (("facebook/dino-vitb8", torch.bfloat16), ("facebook/dino-vitb8", torch.float32), ("facebook/dino-vits8", torch.bfloat16)):
        torch.manual_seed(0)
        model = HookedViT(load_config(name, dtype=dtype, device="cuda")).to(dtype).to(dev).eval()
        images = torch.randn(bs, 3, 224, 224, device=dev, generator=torch.Generator(device=dev).manual_seed(1)).to(dtype)
        tag = f"{name.split('/')[1]}_{'bf16' if dtype == torch.bfloat16 else 'fp32'}"
        native = ms_per_step(model.use_native(True), images, 5)
        assert model.last_run_native
        torch_ms = ms_per_step(model.use_native(False), images, 2)
        model.use_native(True)
        r = {"native_ms_per_step": round(native, 2), "pytorch_ms_per_step": round(torch_ms, 2), "ratio": round(torch_ms / native, 1),
             "attention_us_per_layer_all_hooks": attn_us_per_layer(model, images),
             "attention_us_per_layer_no_taps": attn_us_per_layer(model, images, **z_only)}
        if dtype == torch.bfloat16:
            N.set_tuning("attn_wg", 1)                          # bf16 / d_head 64 on attn_stream_kernel instead of attn_lean_kernel
            r["stream_kernel_us_per_layer_all_hooks"] = attn_us_per_layer(model, images)
            r["stream_kernel_us_per_layer_no_taps"] = attn_us_per_layer(model, images, **z_only)
            N.set_tuning("reset")
        out[tag] = r
        del model, images
        torch.cuda.empty_cache()
print(json.dumps(out))
