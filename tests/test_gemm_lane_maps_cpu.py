"""The lane maps of the bf16 GEMMs on v_mfma_f32_16x16x32_bf16, emulated in numpy (no GPU).

csrc/kloop.hpp and the GEMM kernel files (csrc/gemm_tiled.hpp, csrc/gemm_v4.hpp, csrc/gemm_epi.hpp) state where a DMA piece lands in an LDS slot (swz64 / swz128), which 16 bytes a lane reads as its
A / B fragment, which accumulator registers a 16 x 16 block of the wave's tile occupies, and how the store epilogue walks a 32-row
block in four passes through its 8 x 64 staging rows.  This file restates those formulas and runs one slab of a (64*MB) x 256 tile
through them -- every wave, every lane -- for Ring64 and Ring128 at MB = 4 and 5: the tile must come out as A . B^T with every
element at its own (row, column), and a 16-lane group's ds_read_b128 / the 64 lanes' ds_write_b32 must spread over all 64 banks.

The instruction itself (ISA: A and B fragments row = lane & 15, k = 8 * (lane >> 4) .. + 7; C col = lane & 15,
row = 4 * (lane >> 4) + reg) is the only thing taken as given.
"""
from __future__ import annotations

import numpy as np
import pytest

LANES = np.arange(64)


def swz64(row):
    return (row >> 2) & 3


def swz128(row):
    return (row >> 1) & 7


def fill_slot(src, slab_bytes):
    """What the LDS-DMA leaves in a slot part: src [rows][slab_bytes / 2] elements -> [rows][chunk position][8 elements]."""
    rows = src.shape[0]
    nch = slab_bytes // 16
    slot = np.zeros((rows, nch, 8), dtype=src.dtype)
    rows_per_piece = 1024 // slab_bytes
    for piece in range(rows // rows_per_piece):
        for lane in LANES:
            row = piece * rows_per_piece + lane // nch          # piece_row
            pos = lane % nch                                     # the lane's 16 bytes land at piece base + lane * 16
            sw = swz64(row) if slab_bytes == 64 else swz128(row)
            chunk = pos ^ sw                                     # piece_col: the source column it fetched
            slot[row, pos] = src[row, chunk * 8:chunk * 8 + 8]
    return slot


def read_fragment(slot, slab_bytes, row0, blk, h, lane):
    """rd_a16 / rd_b16: 16-row block blk of the wave's rows (from row0), k-step h, one lane's 8 elements; and its bank group."""
    l15, g = lane & 15, lane >> 4
    row = row0 + blk * 16 + l15
    sw = swz64(l15) if slab_bytes == 64 else swz128(l15)
    pos = (4 * h + g) ^ sw
    byte = row * slab_bytes + pos * 16
    return slot[row, pos], (byte % 256) // 16


def mfma_16x16x32(c, a_frag, b_frag):
    """c [lane][4] += the ISA's layout: a_frag / b_frag [lane][8]."""
    a = np.zeros((16, 32), dtype=np.float64)
    b = np.zeros((16, 32), dtype=np.float64)
    for lane in LANES:
        a[lane & 15, 8 * (lane >> 4):8 * (lane >> 4) + 8] = a_frag[lane]
        b[lane & 15, 8 * (lane >> 4):8 * (lane >> 4) + 8] = b_frag[lane]
    d = a @ b.T
    for lane in LANES:
        for reg in range(4):
            c[lane, reg] += d[4 * (lane >> 4) + reg, lane & 15]


def epi_pass_row(it):
    return (it >> 1) * 16 + (it & 1) * 2


def epi_lane_row(lane):
    j8 = lane >> 3
    return 4 * (j8 >> 1) + (j8 & 1)


def epi_read_off(lane):
    j8, c8 = lane >> 3, lane & 7
    return j8 * 64 + (((c8 >> 1) ^ (j8 >> 1)) * 16 + (c8 & 1) * 8)


def run_wave(A, B, slab_bytes, MB, wave):
    """One wave's (32*MB) x 64 outputs from one slab, through slot, fragments, accumulators and the staged epilogue."""
    wm, wn = wave >> 2, wave & 3
    slotA, slotB = fill_slot(A, slab_bytes), fill_slot(B, slab_bytes)
    # acc[mi][nh][lane][16]: block (m16, nj) is quarter 2 * (m16 & 1) + (nj & 1) of acc[m16 >> 1][nj >> 1]
    acc = np.zeros((MB, 2, 64, 16))
    for h in range(slab_bytes // 64):
        for m16 in range(2 * MB):
            fa = [read_fragment(slotA, slab_bytes, wm * 32 * MB, m16, h, l) for l in LANES]
            for grp in range(4):                                 # a ds_read_b128 is served 16 lanes at a time
                assert sorted(bank for _, bank in fa[16 * grp:16 * grp + 16]) == list(range(16))
            for nj in range(4):
                fb = [read_fragment(slotB, slab_bytes, wn * 64, nj, h, l) for l in LANES]
                for grp in range(4):
                    assert sorted(bank for _, bank in fb[16 * grp:16 * grp + 16]) == list(range(16))
                q = 2 * (m16 & 1) + (nj & 1)
                mfma_16x16x32(acc[m16 >> 1, nj >> 1, :, 4 * q:4 * q + 4], np.array([f for f, _ in fa]),
                              np.array([f for f, _ in fb]))
    out = np.full((32 * MB, 64), np.nan)
    for mi in range(MB):
        for it in range(4):
            stage = np.full(8 * 64, np.nan)
            for nj in range(4):
                for rr in range(2):
                    addr = []
                    for lane in LANES:                           # stage_pass16
                        g, l15 = lane >> 4, lane & 15
                        a = (2 * g + rr) * 64 + ((nj ^ g) * 16 + l15)
                        assert np.isnan(stage[a])
                        stage[a] = acc[mi, nj >> 1, lane, 4 * (2 * (it >> 1) + (nj & 1)) + 2 * (it & 1) + rr]
                        addr.append(a)
                    assert sorted(a % 64 for a in addr) == list(range(64))      # one ds_write_b32: 64 lanes, 64 banks
            for lane in LANES:
                row = mi * 32 + epi_pass_row(it) + epi_lane_row(lane)
                col = (lane & 7) * 8
                off = epi_read_off(lane)
                assert np.isnan(out[row, col])
                out[row, col:col + 8] = stage[off:off + 8]
    return out


@pytest.mark.parametrize("MB", [4, 5])
@pytest.mark.parametrize("slab_bytes", [64, 128])
def test_one_slab_through_slot_fragments_accumulators_and_epilogue(slab_bytes, MB):
    rng = np.random.default_rng(10 * slab_bytes + MB)
    k = slab_bytes // 2
    A = rng.integers(-3, 4, size=(64 * MB, k)).astype(np.float64)
    B = rng.integers(-3, 4, size=(256, k)).astype(np.float64)
    want = A @ B.T
    for wave in (0, 3, 5, 6):        # both wave rows, all four wave columns
        wm, wn = wave >> 2, wave & 3
        got = run_wave(A, B, slab_bytes, MB, wave)
        np.testing.assert_array_equal(got, want[wm * 32 * MB:(wm + 1) * 32 * MB, wn * 64:(wn + 1) * 64])


def test_the_passes_of_a_block_cover_its_32_rows_once():
    rows = sorted(epi_pass_row(it) + epi_lane_row(lane) for it in range(4) for lane in range(0, 64, 8))
    assert rows == list(range(32))
