"""bench.py's command line and its --dump-outputs writer, on the host (the timed path itself runs in test_bench_plain_gpu.py)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_default_and_full_is_an_option(monkeypatch):
    a = parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    a = parse(monkeypatch, "--steps", "3", "--full", "--dump-outputs", "out_dir")
    assert a.steps == 3 and a.full is True and a.dump_outputs == "out_dir"


def test_steps_must_be_positive(monkeypatch):
    with pytest.raises(SystemExit):
        parse(monkeypatch, "--steps", "0")


def test_dump_writes_float32_with_a_fixed_sample_of_large_arrays(tmp_path):
    g = torch.Generator().manual_seed(0)
    out = torch.randn(64, 512, generator=g).to(torch.bfloat16)
    big = torch.randn(16, 12, 50, 50, generator=g).to(torch.bfloat16)
    cache = {"blocks.0.hook_resid_post": torch.randn(4, 50, 64, generator=g), "blocks.0.attn.hook_pattern": big,
             "blocks.0.attn.hook_pattern_view": big.transpose(1, 2)}                     # (a strided view: row-major order of the view)
    written = bench.dump_outputs(str(tmp_path / "a"), out, cache)
    assert sorted(written) == sorted(["output.npy"] + [f"cache.{k}.npy" for k in cache])
    got = {f: np.load(tmp_path / "a" / f) for f in written}
    assert all(v.dtype == np.float32 for v in got.values())
    assert np.array_equal(got["output.npy"], out.float().numpy())                       # small enough: whole, with its shape
    assert np.array_equal(got["cache.blocks.0.hook_resid_post.npy"], cache["blocks.0.hook_resid_post"].numpy())
    s = got["cache.blocks.0.attn.hook_pattern.npy"]
    assert s.shape == (bench.DUMP_SAMPLE,)
    assert np.isin(s, big.float().reshape(-1).numpy()).all()                            # elements of the array, nothing else
    v = got["cache.blocks.0.attn.hook_pattern_view.npy"]
    assert np.isin(v, big.transpose(1, 2).float().reshape(-1).numpy()).all()
    # the same arrays give the same files, whatever was written before
    bench.dump_outputs(str(tmp_path / "b"), out, cache)
    for f in written:
        assert np.array_equal(np.load(tmp_path / "b" / f), got[f]), f
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in written) <= bench.DUMP_MAX_BYTES


def test_dump_sample_positions_depend_on_the_name_only(tmp_path):
    x = torch.arange(200_000, dtype=torch.float32)
    bench.dump_outputs(str(tmp_path / "a"), torch.zeros(2), {"k": x})
    bench.dump_outputs(str(tmp_path / "b"), torch.zeros(2), {"k": x * 2})
    a, b = np.load(tmp_path / "a" / "cache.k.npy"), np.load(tmp_path / "b" / "cache.k.npy")
    assert np.array_equal(a * 2, b) and np.all(np.diff(a) >= 0)                  # same positions, sorted
    assert len(np.unique(a)) > bench.DUMP_SAMPLE * 0.8


def test_dump_refuses_more_than_its_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1000)
    with pytest.raises(RuntimeError, match="dump-outputs"):
        bench.dump_outputs(str(tmp_path), torch.zeros(10), {"k": torch.zeros(1000)})
