"""Reads tests/golden/text_tiny_full.npz and its parts (tests/golden/gen_golden_text.py) back as one mapping, once."""
from __future__ import annotations

import functools
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def text_tiny_full() -> dict:
    """{name: array} of every cache tensor of the reference's fp32 run, plus ``__keys__`` (firing order), ``__out__``, ``__tokens__``."""
    head = np.load(os.path.join(GOLDEN, "text_tiny_full.npz"))
    out = {k: head[k] for k in ("__keys__", "__out__", "__tokens__")}
    for i in range(int(head["__parts__"])):
        part = np.load(os.path.join(GOLDEN, f"text_tiny_full.part{i}.npz"))
        out.update({k: part[k] for k in part.files})
    assert sorted(k for k in out if not k.startswith("__")) == sorted(str(k) for k in out["__keys__"])
    return out


@functools.lru_cache(maxsize=None)
def bf16_budget() -> dict:
    with open(os.path.join(GOLDEN, "text_tiny_bf16_budget.json")) as f:
        return json.load(f)
