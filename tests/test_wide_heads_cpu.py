"""Wide heads (64 < d_head <= 128, d_head % 8 == 0: CLIP ViT-H/14 80, g/14 88, bigG/14 104) without a GPU: what ``NativeViT.supported``
and ``pv_vit_plan_create`` accept and refuse, the loader's entries against the reference's registry, the PyTorch path against the
reference's run of a tiny wide model, and what the compiler makes of ``attn_wide_kernel``.

Fixtures (tests/golden/gen_golden_vit_wide.py, which executes the reference on the CPU):
* ``model_registry_wide.json``   the registry's override fields for the three names (models/model_config_registry.py:253-258, 326-328);
* ``vit_tiny_wide.npz``          the reference's fp32 run of ``synth.ARCHS["tiny-wide"]`` (2 layers, 2 heads of 80, T = 17), batch 3: every
  cache tensor, the key order and the output.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from vit_prisma_amd import HookedViT, HookedViTConfig, _native
from vit_prisma_amd.native_vit import NativeViT
from vit_prisma_amd.synth import ARCHS, synth_images, synth_vit_state

from test_kernel_resources_cpu import _find_hipcc, compile_report, parse_resource_report

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WIDE_NAMES = ["open-clip:laion/CLIP-ViT-H-14-laion2B-s32B-b79K", "open-clip:laion/CLIP-ViT-bigG-14-laion2B-39B-b160k",
              "open-clip:laion/CLIP-ViT-g-14-laion2B-s34B-b88K"]
WIDE_BATCH = 3
LDS_PER_CU = 160 * 1024


def rel_fro(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def wide_tiny_model(dtype=torch.float32, device="cpu") -> HookedViT:
    """``tiny-wide`` from ``synth_vit_state`` seed 0: the model of vit_tiny_wide.npz (shared with tests/test_wide_heads_gpu.py)"""
    arch = ARCHS["tiny-wide"]
    model = HookedViT(HookedViTConfig(**arch, dtype=dtype, device=device))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth_vit_state(arch, seed=0).items()}, strict=True)
    return model.to(dtype).to(device).eval()


def _cfg(d_head, dtype=torch.float32, **kw):
    """one layer, 2 heads of d_head, patch 14 at 224 px: T = 257, the wide models' own"""
    base = dict(ARCHS["tiny"], n_layers=1, n_heads=2, d_head=d_head, d_model=2 * d_head, patch_size=14, image_size=224)
    base.update(kw)
    return HookedViTConfig(**base, dtype=dtype, device="cpu")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("d_head", [72, 80, 88, 96, 104, 128])
def test_native_plan_accepts_wide_heads(d_head, dtype):
    assert NativeViT.supported(_cfg(d_head, dtype), 257) is None


@pytest.mark.parametrize("name", WIDE_NAMES)
def test_native_plan_accepts_the_three_registry_names(name):
    from vit_prisma_amd.model_loader import load_config
    for dtype in (torch.float32, torch.bfloat16):
        cfg = load_config(name, device="cpu", dtype=dtype)
        T = (cfg.image_size // cfg.patch_size) ** 2 + 1
        assert T == 257 and NativeViT.supported(cfg, T) is None, (name, dtype)


@pytest.mark.parametrize("d_head", [48, 76, 136])
def test_native_plan_refuses_other_head_widths(d_head):
    assert NativeViT.supported(_cfg(d_head), 257) == "attention shape"


def test_native_plan_refuses_a_wide_head_beyond_the_token_cap():
    assert NativeViT.supported(_cfg(80), 2048) is None
    assert NativeViT.supported(_cfg(80), 2049) == "attention shape"


def _desc(d_head):
    return _native.VitDesc(n_layers=1, d_model=2 * d_head, n_heads=2, d_head=d_head, d_mlp=128, n_channels=3, patch_size=4, image_size=16,
                           n_tokens=17, n_classes=24, use_cls_token=1, layer_norm_pre=1, has_head=1, normalize_output=1, activation=0,
                           dtype=0, eps=1e-5, attn_scale=d_head ** 0.5, pooling=0)


def test_plan_creation_accepts_wide_heads_and_states_the_rule_when_it_refuses():
    lib = _native.lib()
    assert lib.pv_abi_version() == _native.ABI_VERSION == 26
    plan = C.c_void_p()
    for d_head in (80, 104):
        desc = _desc(d_head)
        assert lib.pv_vit_plan_create(C.byref(desc), C.byref(plan)) == 0, (d_head, _native.last_error())
        lib.pv_vit_plan_destroy(plan)
    for d_head in (136, 76):
        desc = _desc(d_head)
        assert lib.pv_vit_plan_create(C.byref(desc), C.byref(plan)) == 1, d_head
        why = _native.last_error()
        assert "64 < d_head <= 128" in why and "d_head % 8 == 0" in why and "{32, 64}" in why and "2048" in why, why


def test_wide_registry_entries_equal_the_reference_registry():
    from vit_prisma_amd.model_loader import WIDE_ARCH, list_available_models, load_config
    with open(os.path.join(GOLDEN, "model_registry_wide.json")) as f:
        reg = json.load(f)
    assert sorted(reg) == sorted(WIDE_ARCH) == sorted(WIDE_NAMES)
    for name, fields in reg.items():
        assert name in list_available_models()
        cfg = load_config(name, device="cpu")
        assert cfg.model_name == name and cfg.d_head == cfg.d_model // cfg.n_heads
        assert fields, name
        for k, v in fields.items():
            assert getattr(cfg, k) == v, (name, k, getattr(cfg, k), v)
    # open_clip's published model configs
    want = {WIDE_NAMES[0]: (32, 1280, 80, 5120, 1024), WIDE_NAMES[2]: (40, 1408, 88, 6144, 1024), WIDE_NAMES[1]: (48, 1664, 104, 8192, 1280)}
    for name, dims in want.items():
        cfg = load_config(name, device="cpu")
        assert (cfg.n_layers, cfg.d_model, cfg.d_head, cfg.d_mlp, cfg.n_classes) == dims, name
        assert (cfg.patch_size, cfg.image_size, cfg.n_heads, cfg.activation_name) == (14, 224, 16, "gelu"), name


def test_wide_tiny_model_on_the_pytorch_path_vs_reference_fixture():
    """Passes without the wide-head kernel: it pins the fixture the GPU test holds the HIP plan to."""
    G = np.load(os.path.join(GOLDEN, "vit_tiny_wide.npz"))
    arch = ARCHS["tiny-wide"]
    assert (arch["n_layers"], arch["d_model"], arch["n_heads"], arch["d_head"], arch["d_mlp"]) == (2, 160, 2, 80, 192)
    model = wide_tiny_model()
    with torch.no_grad():
        out, cache = model.run_with_cache(torch.from_numpy(synth_images(arch, WIDE_BATCH, 1)))
    keys = [str(k) for k in G["__keys__"]]
    assert list(cache.keys()) == keys
    assert cache["blocks.0.attn.hook_z"].shape == (WIDE_BATCH, 17, 2, 80)
    for k in keys:
        assert cache[k].shape == G[k].shape and rel_fro(cache[k], torch.from_numpy(G[k])) < 1e-4, k
    assert out.shape == (WIDE_BATCH, 16) and rel_fro(out, torch.from_numpy(G["__out__"])) < 1e-4


# instance -> (source, mangled name up to the argument list, least waves per SIMD the header comment of attention_wide.hip states).
# t = unsigned short = bf16 storage, f = float.  fp32: z alone is 48 / 64 accumulator registers beside the Q fragments: one workgroup
# per CU; bf16: 60 / 69 KiB of LDS = two workgroups per CU.  The resume kernel keeps its floor (test_attention_long_resources_cpu).
EXPECTED = {
    "attn_wide_kernel<float, 96>": ("attention_wide.hip", "16attn_wide_kernelIfLi96EEEv", 1),
    "attn_wide_kernel<float, 128>": ("attention_wide.hip", "16attn_wide_kernelIfLi128EEEv", 1),
    "attn_wide_kernel<bf16, 96>": ("attention_wide.hip", "16attn_wide_kernelItLi96EEEv", 2),
    "attn_wide_kernel<bf16, 128>": ("attention_wide.hip", "16attn_wide_kernelItLi128EEEv", 2),
    "attn_resume_kernel<float>": ("attention.hip", "18attn_resume_kernelIfEEv", 4),
    "attn_resume_kernel<bf16>": ("attention.hip", "18attn_resume_kernelItEEv", 4),
}


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    import concurrent.futures as cf
    hipcc = _find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc: the resource report needs the ROCm compiler")
    outdir = str(tmp_path_factory.mktemp("kernel_resources_wide"))
    sources = ("attention_wide.hip", "attention.hip")
    with cf.ThreadPoolExecutor(max_workers=len(sources)) as ex:
        reports = list(ex.map(lambda s: compile_report(hipcc, s, outdir), sources))
    table = {}
    for src, text in zip(sources, reports):
        parsed = parse_resource_report(text)
        assert parsed, f"{src}: hipcc printed no kernel-resource-usage remarks"
        for mangled, res in parsed.items():
            table[(src, mangled)] = res
    return table


@pytest.mark.parametrize("kernel", sorted(EXPECTED))
def test_wide_attention_kernels_scratch_lds_and_waves(resources, kernel):
    src, fragment, floor = EXPECTED[kernel]
    hits = [k for k in resources if k[0] == src and fragment in k[1]]
    assert len(hits) == 1, f"{kernel} ({fragment}) is not among the kernels {src} compiles to: {sorted(m for s_, m in resources if s_ == src)}"
    got = resources[hits[0]]
    print(f"{kernel}: {got}")
    assert got["scratch"] == 0, f"{kernel} spills to scratch: {got}"
    assert got["lds"] <= LDS_PER_CU, f"{kernel}: {got['lds']} bytes of LDS per workgroup: {got}"
    by_lds = LDS_PER_CU // got["lds"] if got["lds"] else 8
    waves = min(got["occupancy"], by_lds)
    assert waves >= floor, f"{kernel}: {waves} waves per SIMD (registers {got['occupancy']}, LDS {by_lds}), the design states >= {floor}: {got}"


def test_every_instance_of_the_wide_kernel_is_listed(resources):
    listed = {v[1] for v in EXPECTED.values()}
    wide = [m for _, m in resources if "attn_wide_kernel" in m]
    assert len(wide) == 4, wide
    for mangled in wide:
        assert any(f in mangled for f in listed), f"{mangled} has no entry in EXPECTED"
        assert not any(n in mangled for n in ("attn_stream_kernel", "attn_resume_kernel", "token_mean_kernel")), mangled
