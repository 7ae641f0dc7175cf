// The main loop of the one-workgroup-per-CU MFMA kernels (gfx950): gemm_kernel_v7 / gemm_kernel_v8 (gemm.hip, bf16) and
// sae_enc_gemm_kernel (sae_enc_gemm.hip, fp16).  One 512-thread workgroup (8 waves as 2 (M) x 4 (N)) multiplies a (64*MB) x 256 tile;
// a wave owns (32*MB) x 64 outputs = MB x 2 accumulators of f32x16, multiplied on v_mfma_f32_16x16x32_bf16 (bf16: 2*MB x 4 blocks,
// four to an accumulator) or v_mfma_f32_32x32x16_f16 (fp16): the shape belongs to the operand tag, see Shape below.  The operands are DMA'd straight into LDS
// (buffer_load ... lds) in PIECES of 1 KiB = one wave-instruction; wave w moves pieces w, w + 8, ... of a slab's A part and of its
// B part.  What is here, once:
//   * the tile order (virtual block id -> tile), TileOrder
//   * the geometry of a ring slot -- which LDS address a piece lands at, which source column a lane fetches, where a lane reads
//     its MFMA fragments -- for 64-byte K slabs (Ring64) and for 128-byte ones (Ring128)
//   * the three K-loop forms with their drivers (prologue issues, ring-unrolled loop, tails):
//       KLOOP_RUN_FETCH_AFTER_BARRIER 64-byte slabs, four slots; any A operand, K tails             (LP = 0)
//       KLOOP_RUN_PIPELINED64         64-byte slabs, four slots, software-pipelined                 (LP = 1)
//       KLOOP_RUN_FULL_LINE           128-byte slabs (whole cache lines), two slots                 (LP = 2)
//     and step_full_line on its own for the persistent kernel, whose driver walks tiles.
// What a user supplies: the MFMA operand type (Bf16 / F16), MB, its __shared__ slot objects, its two buffer descriptors and a
// SOURCE FUNCTOR  src(kt, j) -> byte offset into the A (j < pieces of A) or B descriptor of the piece j this wave moves for slab kt,
// or DEAD (LP = 0: a functor per slab, see there).  That functor is where the users differ: plain rows, the patch gather, a K
// tail, an explicit N bound, a slab index that runs into the next tile.
//
// Three rules every line below keeps (each was paid for with a drained DMA queue):
//   * SELECTS, NOT BRANCHES, around an LDS-DMA: hipcc's waitcnt pass answers a conditionally executed LDS-DMA with
//     s_waitcnt vmcnt(0) before the next ds_read.  A piece that must not load gets the offset DEAD (past every descriptor's range:
//     the DMA zero-fills); source functors use bitwise |, & so that their conditions compile to selects.
//   * ONE __shared__ OBJECT PER SLOT, declared by the kernel and handed in as pointers: hipcc's alias scopes are per LDS variable.
//     Only then can it prove that the ds_reads of one slot do not alias the DMA writes in flight to the others; with a single
//     array it waits vmcnt(0) before the first ds_read of every step.  (These functions are force-inlined into the kernel, so the
//     pointers are the objects again by the time that pass runs.)
//   * THE ISSUE ORDER IS THE SCHEDULE in the pipelined forms: MFMA group | DMA piece + fragment refill | MFMA group | ..., pinned
//     with sched_barrier (a group: one A fragment against the wave's B fragments, 2 MFMAs of 32x32x16 or 4 of 16x16x32).  Left to itself hipcc sinks the refills to the end of the (half-)slab and waits for them right behind the
//     barrier, with the matrix pipe idle.
// The waits are COUNTED s_waitcnt vmcnt(n) across a raw s_barrier (simm16 0x0F70 | n: expcnt 7, lgkmcnt 15 -- only vmcnt is waited
// on): __syncthreads() would drain the queue.  Every wave retires the same number of pieces per slab, so n is a compile-time figure.
#pragma once
#include "pv_common.hpp"

namespace kloop {

typedef __attribute__((address_space(3))) void* lds_ptr_t;      // destination of an LDS-DMA
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
constexpr unsigned DEAD = 0xffffff00u;                          // source offset of a piece that must not load

// operand-type tags
struct Bf16 {};
struct F16 {};
__device__ __forceinline__ f32x16 mfma(Bf16, const uint4& a, const uint4& b, const f32x16& c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma(F16, const uint4& a, const uint4& b, const f32x16& c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
// The MFMA shape belongs to the operand tag.  Bf16 multiplies on v_mfma_f32_16x16x32_bf16 (S16): the wave's (32*MB) x 64 outputs
// are then 2*MB x 4 accumulators of f32x4 (C layout: col = lane & 15, row = 4 * (lane >> 4) + reg), a k-step is 32 elements = 64
// bytes of K, and a fragment is still one ds_read_b128: lane l takes row l & 15 of its 16-row block at chunk 4 * h + (l >> 4) of
// the slab row.  Same flops per cycle, same LDS reads per slab as 32x32x16 -- but under the socket's power cap the chip holds a
// higher clock on this shape.  -DPV_GEMM_MFMA=32 compiles the 32x32x16 shape into every bf16 kernel (A/B builds);
// F16 (the SAE filter GEMM) is on 32x32x16.
#ifndef PV_GEMM_MFMA
#define PV_GEMM_MFMA 16
#endif
static_assert(PV_GEMM_MFMA == 16 || PV_GEMM_MFMA == 32, "PV_GEMM_MFMA: 16 (16x16x32) or 32 (32x32x16)");
template <class OP> struct Shape { static constexpr bool S16 = false; };
template <> struct Shape<Bf16> { static constexpr bool S16 = PV_GEMM_MFMA == 16; };
// The accumulators stay f32x16 [MB][2] for both shapes.  S16: the 16 x 16 block (16-row block m16 < 2 * MB, 16-column block
// nj < 4) of the wave's tile is the QUARTER 2 * (m16 & 1) + (nj & 1) -- four consecutive registers -- of acc[m16 >> 1][nj >> 1].
// (Not f32x4 [2 * MB][4]: v_mfma_f32_16x16x32 does not tie its destination to its C operand, and with 40 separate four-register
// values hipcc's register allocator rotates the accumulators through the loop and spills; as a quarter of a sixteen-register
// value a block has nowhere else to go.)
__device__ __forceinline__ void mfma16_at(Bf16, f32x16& acc, int q, const uint4& a, const uint4& b) {
    f32x4 c = {acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[4 * q + i] = c[i];
}
// ... which the compiler may have to be told: with every index a constant it takes the sixteen-register values apart again.  An
// empty asm that names each accumulator as ONE operand keeps them whole where it stands (no instruction).  The persistent kernel
// needs it at the head of every slab (without: 52 - 100 VGPRs spilled at MB = 5); the drivers below place it around their tail
// steps, where the accumulators of the loop and of the tail meet (without: 14 registers more at MB = 5, the residual epilogue
// spills); at the head of every step the one-tile kernels are worse off with it.
template <int MB>
__device__ __forceinline__ void keep_whole(f32x16 (&acc)[MB][2]) {
#pragma unroll
    for (int mi = 0; mi < MB; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) asm volatile("" : "+v"(acc[mi][ni]));
}
template <class OP, int MB>
__device__ __forceinline__ void keep_whole_if_s16(f32x16 (&acc)[MB][2]) {
    if constexpr (Shape<OP>::S16) keep_whole(acc);
}
// S16: one A fragment (16-row block m16) against the wave's four B fragments (fb[nj >> 1][nj & 1])
template <class OP, int MB>
__device__ __forceinline__ void mfma_quad(f32x16 (&acc)[MB][2], int m16, const uint4& a, const uint4 (&b01)[2], const uint4 (&b23)[2]) {
    const int q = 2 * (m16 & 1);
    mfma16_at(OP{}, acc[m16 >> 1][0], q, a, b01[0]);
    mfma16_at(OP{}, acc[m16 >> 1][0], q + 1, a, b01[1]);
    mfma16_at(OP{}, acc[m16 >> 1][1], q, a, b23[0]);
    mfma16_at(OP{}, acc[m16 >> 1][1], q + 1, a, b23[1]);
}
// one A fragment against the wave's two B fragments
template <class OP>
__device__ __forceinline__ void mfma_pair(f32x16 (&acc)[2], const uint4& a, const uint4 (&b)[2]) {
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) acc[ni] = mfma(OP{}, a, b[ni], acc[ni]);
}

__device__ __forceinline__ void dma16(const __amdgpu_buffer_rsrc_t& rs, unsigned char* dst, unsigned off) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr_t)dst, 16, off, 0, 0, 0);
}
__device__ __forceinline__ void pin() { __builtin_amdgcn_sched_barrier(0); }

// One piece of a full-line slab through the source functor.  A functor is  src(kt, j) -> offset  and the piece goes where
// Ring128::issue puts it; one that has a member  piece(g, rsA, rsB, slotA, slotB, kt, j)  places the piece itself -- descriptor,
// source and destination inside the slot it is handed (gemm.hip's residual park: the DEAD pieces off the end of the loop get a real
// source there).  Same rules: selects only, and the destination stays inside the slot object of the call.
template <class G, class Src>
__device__ __forceinline__ auto issue_piece(int, const G& g, const __amdgpu_buffer_rsrc_t& rsA, const __amdgpu_buffer_rsrc_t& rsB,
                                            unsigned char* slotA, unsigned char* slotB, int kt, int j, const Src& src)
    -> decltype(src.piece(g, rsA, rsB, slotA, slotB, kt, j)) {
    return src.piece(g, rsA, rsB, slotA, slotB, kt, j);
}
template <class G, class Src>
__device__ __forceinline__ void issue_piece(long, const G& g, const __amdgpu_buffer_rsrc_t& rsA, const __amdgpu_buffer_rsrc_t& rsB,
                                            unsigned char* slotA, unsigned char* slotB, int kt, int j, const Src& src) {
    g.issue(rsA, rsB, slotA, slotB, j, src(kt, j));
}

// ---------------------------------------------------------------------------------------------------
// Tile order.  Block b of a launch runs on XCD b % 8: xcd_run() is the bijection that gives each XCD a contiguous run of the
// linear order, so that neighbours in that order share an L2.  (A persistent kernel passes its virtual block id and the tile
// count: vb and vb + k * grid sit on the same XCD.)
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ int xcd_run(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}
// The linear order itself: column blocks of <= 8 N-tiles, M-major inside a block.  The B panel of a block (8 x TN rows x K) stays
// resident in the XCD's 4 MB L2 while the M range streams past once per block, instead of the whole weight matrix being
// re-streamed every few M-tiles (PMC: L2-miss reads were 4x the algorithmic bytes with plain N-fastest order).
template <int TM, int TN>
struct TileOrder {
    int ntn, ntm, wblk;
    __device__ __forceinline__ TileOrder(int M, int N) {
        ntn = (N + TN - 1) / TN;
        ntm = (M + TM - 1) / TM;
        const int nblk = (ntn + 7) / 8;
        wblk = (ntn + nblk - 1) / nblk;
    }
    // position swz in the order -> tile
    __device__ __forceinline__ void at(int swz, int& tile_m, int& tile_n) const {
        const int blk = swz / (ntm * wblk);
        const int rem = swz - blk * (ntm * wblk);
        const int wcur = min(wblk, ntn - blk * wblk);
        tile_m = rem / wcur;
        tile_n = blk * wblk + (rem - tile_m * wcur);
    }
};

// ---------------------------------------------------------------------------------------------------
// Slot of 64-byte K slabs: (64*MB + 256) rows x 64 B, the A rows first.  A row is 4 chunks of 16 B and 4 rows share a 256-byte
// bank row; chunk c of row r sits at position c ^ swz64(r), applied on the DMA source column and on the fragment reads
// (conflict-free ds_read_b128).  A piece is 16 rows; per slab a wave issues NA = ceil(4*MB / 8) A pieces + 2 B pieces.  At MB = 5
// waves 4..7 have only 2 real A pieces -- their third is a DEAD DMA into a pad, so that every wave retires the same number.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ int swz64(int row) { return (row >> 2) & 3; }

template <int MB, bool S16 = false>
struct Ring64 {
    static constexpr int A_BYTES = 64 * MB * 64, B_BYTES = 256 * 64, SLOT = A_BYTES + B_BYTES;
    static constexpr int NA = (4 * MB + 7) / 8;
    static constexpr bool PAD = (4 * MB) % 8 != 0;
    static constexpr int PAD_BYTES = PAD ? 8192 : 16;
    static constexpr int NPIECE = NA + 2;                 // pieces per wave per slab
    static constexpr int PIECE_STRIDE = 128;              // rows between a wave's consecutive pieces
    static_assert(4 * SLOT + PAD_BYTES <= 160 * 1024, "one workgroup per CU");
    static_assert(3 * NPIECE <= 15, "the vmcnt immediates use the low 4 bits only");
    int wave;
    unsigned char* pad;
    int a_row, b_row, co0, co1;
    __device__ __forceinline__ Ring64(int lane, int wave_, unsigned char* pad_) : wave(wave_), pad(pad_) {
        if constexpr (S16) {
            // (blocks start at multiples of 16 rows: the swizzle of a fragment row is that of l & 15)
            const int l15 = lane & 15;
            co0 = co1 = ((lane >> 4) ^ swz64(l15)) * 16;
            a_row = ((wave >> 2) * 32 * MB + l15) * 64;
            b_row = A_BYTES + ((wave & 3) * 64 + l15) * 64;
        } else {
            const int l31 = lane & 31, half = lane >> 5, sw = swz64(l31);
            co0 = ((0 + half) ^ sw) * 16;
            co1 = ((2 + half) ^ sw) * 16;
            a_row = ((wave >> 2) * 32 * MB + l31) * 64;
            b_row = A_BYTES + ((wave & 3) * 64 + l31) * 64;
        }
    }
    // the row (of the slab's A or B part) and the source byte column that this lane fetches for this wave's piece j
    __device__ __forceinline__ int piece_row(int lane, int j) const { return (j * 8 + wave) * 16 + (lane >> 2); }
    __device__ static __forceinline__ int piece_col(int lane, int row) { return ((lane & 3) ^ swz64(row)) * 16; }
    __device__ __forceinline__ bool real_a(int j) const { return j * 8 + wave < 4 * MB; }      // (uniform)
    // piece j of a slab (j < NA: of A, else of B) from source offset `off` into `slot`
    __device__ __forceinline__ void issue(const __amdgpu_buffer_rsrc_t& rsA, const __amdgpu_buffer_rsrc_t& rsB, unsigned char* slot,
                                          int j, unsigned off) const {
        if (j < NA) {
            unsigned char* dst = slot + (j * 8 + wave) * 1024;
            if constexpr (PAD) { if (j == NA - 1) dst = real_a(j) ? dst : pad + wave * 1024; }
            dma16(rsA, dst, off);
        } else {
            dma16(rsB, slot + A_BYTES + ((j - NA) * 8 + wave) * 1024, off);
        }
    }
    // fragments of half-slab h (32 bytes of K): block mi of A, block ni of B
    __device__ __forceinline__ uint4 rd_a(const unsigned char* slot, int h, int mi) const {
        return *reinterpret_cast<const uint4*>(slot + a_row + mi * 2048 + (h == 0 ? co0 : co1));
    }
    __device__ __forceinline__ uint4 rd_b(const unsigned char* slot, int h, int ni) const {
        return *reinterpret_cast<const uint4*>(slot + b_row + ni * 2048 + (h == 0 ? co0 : co1));
    }
    // S16: fragments of the slab's one k-step, 16-row block mi of A (< 2 * MB), ni of B (< 4)
    __device__ __forceinline__ uint4 rd_a16(const unsigned char* slot, int mi) const {
        return *reinterpret_cast<const uint4*>(slot + a_row + mi * 1024 + co0);
    }
    __device__ __forceinline__ uint4 rd_b16(const unsigned char* slot, int ni) const {
        return *reinterpret_cast<const uint4*>(slot + b_row + ni * 1024 + co0);
    }
};

// all pieces of slab kt into `slot` (source functor)
template <int MB, bool S16, class Src>
__device__ __forceinline__ void issue_slab64(const Ring64<MB, S16>& g, const __amdgpu_buffer_rsrc_t& rsA, const __amdgpu_buffer_rsrc_t& rsB,
                                             int kt, unsigned char* slot, const Src& src) {
#pragma unroll
    for (int j = 0; j < Ring64<MB>::NPIECE; ++j) g.issue(rsA, rsB, slot, j, src(kt, j));
}

// The steps below come twice: for the 32x32x16 shape and, behind each, for S16.
// The two walk a slab at the same pace -- a GROUP is one A fragment against all of the wave's B fragments, 2 MFMAs there and 4
// here, the same matrix-pipe time -- and keep barriers and DMA pieces behind the same groups.  What differs is the fragment
// registers.  32x32x16: MB A fragments + 2 x 2 B fragments, B double-buffered per 16-element k-step.  S16: the same 36 registers
// hold a ring of MB A fragments (fragment mi lives in fa[mi % MB] and is refilled with fragment mi + MB right behind its group:
// five groups of prefetch distance) and the k-step's four B fragments (fb[ni >> 1][ni & 1]), which are live through all 2 * MB
// groups and refilled from the next k-step behind the last one.

// LP = 0, barrier-then-fetch.  Slab kt+3 is issued (into nxt3, the slot multiplied in step kt-1) while slab kt (in cur) is
// multiplied; at step kt slab kt must have landed, the 2 * NPIECE pieces of slabs kt+1, kt+2 stay in flight across the barrier.
// This form takes the patch gather and K tails, whose sources have terms per slab: its functor is  issue(kt, slot), which puts
// all NPIECE pieces of slab kt into the slot through g.issue().
template <class OP, int MB, class Issue>
__device__ __forceinline__ void step_fetch_after_barrier(f32x16 (&acc)[MB][2], const Ring64<MB>& g, int kt, unsigned char* cur,
                                                         unsigned char* nxt3, const Issue& issue) {
    __builtin_amdgcn_s_waitcnt(0x0F70 | (2 * Ring64<MB>::NPIECE));
    __builtin_amdgcn_s_barrier();
    issue(kt + 3, nxt3);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        uint4 a[MB], b[2];
#pragma unroll
        for (int mi = 0; mi < MB; ++mi) a[mi] = g.rd_a(cur, h, mi);
        b[0] = g.rd_b(cur, h, 0);
        b[1] = g.rd_b(cur, h, 1);
#pragma unroll
        for (int mi = 0; mi < MB; ++mi) mfma_pair<OP>(acc[mi], a[mi], b);
    }
}

template <class OP, int MB, class Issue>
__device__ __forceinline__ void step_fetch_after_barrier(f32x16 (&acc)[MB][2], const Ring64<MB, true>& g, int kt, unsigned char* cur,
                                                         unsigned char* nxt3, const Issue& issue) {
    __builtin_amdgcn_s_waitcnt(0x0F70 | (2 * Ring64<MB>::NPIECE));
    __builtin_amdgcn_s_barrier();
    issue(kt + 3, nxt3);
    uint4 b[2][2];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) b[ni >> 1][ni & 1] = g.rd_b16(cur, ni);
    uint4 a[MB];
#pragma unroll
    for (int mi = 0; mi < MB; ++mi) a[mi] = g.rd_a16(cur, mi);
#pragma unroll
    for (int mi = 0; mi < MB; ++mi) {
        mfma_quad<OP>(acc, mi, a[mi], b[0], b[1]);
        pin();
        a[mi] = g.rd_a16(cur, MB + mi);       // (pinned: hoisted to the top, the second half's fragments cost 20 registers)
        pin();
    }
#pragma unroll
    for (int mi = 0; mi < MB; ++mi) mfma_quad<OP>(acc, MB + mi, a[mi], b[0], b[1]);
}

// LP = 1, software-pipelined.  The loop above has every wave arrive at the slab's barrier with empty fragment registers: both
// waves of a SIMD then issue their DMA pieces and their first ds_reads and sit out the LDS latency with the matrix pipe idle.
// Here the fragments of a half-slab are fetched while the previous half-slab is multiplied (each A fragment is refilled right
// behind the two MFMAs that consumed it), the barrier of slab s+1 sits in the MIDDLE of step s (between its two halves: by then
// every read of slab s has been issued, and the second half's operands are already in registers), and the DMA pieces of slab s+4
// go out one per MFMA pair during the second half, into the slot the barrier has just freed.  Ring depth as before: at the barrier
// of slab s+1 the pieces of slabs s+2 and s+3 stay in flight.  Whole 64-byte slabs only.
//   step kt: slab kt in cur (visible), slab kt+1 in nxt; fa / fb0 hold the first half of slab kt
template <class OP, int MB, class Src>
__device__ __forceinline__ void step_pipelined64(f32x16 (&acc)[MB][2], uint4 (&fa)[MB], uint4 (&fb0)[2], uint4 (&fb1)[2],
                                                 const Ring64<MB>& g, const __amdgpu_buffer_rsrc_t& rsA,
                                                 const __amdgpu_buffer_rsrc_t& rsB, int kt, unsigned char* cur, unsigned char* nxt,
                                                 const Src& src) {
    constexpr int NPIECE = Ring64<MB>::NPIECE;
    static_assert(NPIECE <= MB && MB >= 2, "one DMA piece per MFMA pair; the B refill rides behind pair 1");
#pragma unroll
    for (int mi = 0; mi < MB; ++mi) {
        mfma_pair<OP>(acc[mi], fa[mi], fb0);
        pin();
        fa[mi] = g.rd_a(cur, 1, mi);
        if (mi == 1) { fb1[0] = g.rd_b(cur, 1, 0); fb1[1] = g.rd_b(cur, 1, 1); }
        pin();
    }
    __builtin_amdgcn_s_waitcnt(0x0F70 | (2 * NPIECE));
    __builtin_amdgcn_s_barrier();
    pin();
#pragma unroll
    for (int mi = 0; mi < MB; ++mi) {
        mfma_pair<OP>(acc[mi], fa[mi], fb1);
        pin();
        fa[mi] = g.rd_a(nxt, 0, mi);
        if (mi == 1) { fb0[0] = g.rd_b(nxt, 0, 0); fb0[1] = g.rd_b(nxt, 0, 1); }
        if (mi < NPIECE) g.issue(rsA, rsB, cur, mi, src(kt + 4, mi));
        pin();
    }
}
// S16.  step kt: fa holds A fragments 0 .. MB-1 of slab kt, fb0 / fb1 its B fragments 0, 1 / 2, 3
template <class OP, int MB, class Src>
__device__ __forceinline__ void step_pipelined64(f32x16 (&acc)[MB][2], uint4 (&fa)[MB], uint4 (&fb0)[2], uint4 (&fb1)[2],
                                                 const Ring64<MB, true>& g, const __amdgpu_buffer_rsrc_t& rsA,
                                                 const __amdgpu_buffer_rsrc_t& rsB, int kt, unsigned char* cur, unsigned char* nxt,
                                                 const Src& src) {
    constexpr int NPIECE = Ring64<MB>::NPIECE;
    static_assert(NPIECE <= MB, "one DMA piece per MFMA group");
#pragma unroll
    for (int mi = 0; mi < MB; ++mi) {
        mfma_quad<OP>(acc, mi, fa[mi], fb0, fb1);
        pin();
        fa[mi] = g.rd_a16(cur, MB + mi);
        pin();
    }
    __builtin_amdgcn_s_waitcnt(0x0F70 | (2 * NPIECE));
    __builtin_amdgcn_s_barrier();
    pin();
#pragma unroll
    for (int mi = 0; mi < MB; ++mi) {
        mfma_quad<OP>(acc, MB + mi, fa[mi], fb0, fb1);
        pin();
        fa[mi] = g.rd_a16(nxt, mi);
        if (mi == MB - 1) {
            fb0[0] = g.rd_b16(nxt, 0); fb0[1] = g.rd_b16(nxt, 1);
            fb1[0] = g.rd_b16(nxt, 2); fb1[1] = g.rd_b16(nxt, 3);
        }
        if (mi < NPIECE) g.issue(rsA, rsB, cur, mi, src(kt + 4, mi));
        pin();
    }
}
// its prologue: four slabs issued, slab 0 landed, the first half of slab 0 in the fragment registers
template <int MB, bool S16, class Src>
__device__ __forceinline__ void prologue_pipelined64(uint4 (&fa)[MB], uint4 (&fb0)[2], uint4 (&fb1)[2], const Ring64<MB, S16>& g,
                                                     const __amdgpu_buffer_rsrc_t& rsA, const __amdgpu_buffer_rsrc_t& rsB,
                                                     unsigned char* r0, unsigned char* r1, unsigned char* r2, unsigned char* r3,
                                                     const Src& src) {
    issue_slab64(g, rsA, rsB, 0, r0, src);
    issue_slab64(g, rsA, rsB, 1, r1, src);
    issue_slab64(g, rsA, rsB, 2, r2, src);
    issue_slab64(g, rsA, rsB, 3, r3, src);
    __builtin_amdgcn_s_waitcnt(0x0F70 | (3 * Ring64<MB>::NPIECE));
    __builtin_amdgcn_s_barrier();
    if constexpr (S16) {
#pragma unroll
        for (int mi = 0; mi < MB; ++mi) fa[mi] = g.rd_a16(r0, mi);
        fb0[0] = g.rd_b16(r0, 0); fb0[1] = g.rd_b16(r0, 1);
        fb1[0] = g.rd_b16(r0, 2); fb1[1] = g.rd_b16(r0, 3);
    } else {
#pragma unroll
        for (int mi = 0; mi < MB; ++mi) fa[mi] = g.rd_a(r0, 0, mi);
        fb0[0] = g.rd_b(r0, 0, 0);
        fb0[1] = g.rd_b(r0, 0, 1);
    }
}

// ---------------------------------------------------------------------------------------------------
// Slot of 128-byte K slabs: whole cache lines -- a piece is 8 rows x 128 B = 8 lines instead of 16 half lines (64-byte slabs pull
// every operand line through the L1 twice, 1 us apart, and the texture addresser is busy 55-79 % of the launch:
// profiles/r02_notes.md).  A row is 8 chunks; chunk c of row r at position c ^ swz128(r): the 16 rows of a ds_read_b128 lane group
// (8 even, 8 odd) then cover all 64 banks.  Per slab a wave issues MB A pieces + 4 B pieces.
// SPLIT: the A and the B part of a slot are separate __shared__ objects (the persistent kernel); else the B part follows the A
// part in one object and both slot pointers of a call are that object.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ int swz128(int row) { return (row >> 1) & 7; }

template <int MB, bool SPLIT = false, bool S16 = false>
struct Ring128 {
    static constexpr int A_BYTES = 64 * MB * 128, B_BYTES = 256 * 128, SLOT = A_BYTES + B_BYTES;
    static constexpr int B_BASE = SPLIT ? 0 : A_BYTES;
    static constexpr int NPIECE = MB + 4;                 // pieces per wave per slab
    static constexpr int PIECE_STRIDE = 64;               // rows between a wave's consecutive pieces
    static_assert(MB >= 2, "the B refill rides behind MFMA pair 1");
    int wave;
    int a_row, b_row, fco[4];
    __device__ __forceinline__ Ring128(int lane, int wave_) : wave(wave_) {
        if constexpr (S16) {
            const int l15 = lane & 15, fsw = swz128(l15);
            a_row = ((wave >> 2) * 32 * MB + l15) * 128;
            b_row = B_BASE + ((wave & 3) * 64 + l15) * 128;
#pragma unroll
            for (int h = 0; h < 4; ++h) fco[h] = ((4 * (h & 1) + (lane >> 4)) ^ fsw) * 16;      // (k-steps 0, 1)
        } else {
            const int l31 = lane & 31, half = lane >> 5, fsw = swz128(l31);
            a_row = ((wave >> 2) * 32 * MB + l31) * 128;
            b_row = B_BASE + ((wave & 3) * 64 + l31) * 128;
#pragma unroll
            for (int h = 0; h < 4; ++h) fco[h] = ((2 * h + half) ^ fsw) * 16;
        }
    }
    // the row (of the slab's A or B part) and the source byte column that this lane fetches for this wave's piece 0
    __device__ __forceinline__ int piece_row(int lane) const { return wave * 8 + (lane >> 3); }
    __device__ __forceinline__ unsigned piece_col(int lane) const { return (unsigned)(((lane & 7) ^ swz128(piece_row(lane))) * 16); }
    // piece j of a slab (j < MB: of A, else of B) from source offset `off` into the slot
    __device__ __forceinline__ void issue(const __amdgpu_buffer_rsrc_t& rsA, const __amdgpu_buffer_rsrc_t& rsB, unsigned char* slotA,
                                          unsigned char* slotB, int j, unsigned off) const {
        if (j < MB) dma16(rsA, slotA + (j * 8 + wave) * 1024, off);
        else dma16(rsB, slotB + B_BASE + ((j - MB) * 8 + wave) * 1024, off);
    }
    // fragments of k-step h (16 elements of K): block mi of A, block ni of B
    __device__ __forceinline__ uint4 rd_a(const unsigned char* slotA, int h, int mi) const {
        return *reinterpret_cast<const uint4*>(slotA + a_row + mi * 4096 + fco[h]);
    }
    __device__ __forceinline__ uint4 rd_b(const unsigned char* slotB, int h, int ni) const {
        return *reinterpret_cast<const uint4*>(slotB + b_row + ni * 4096 + fco[h]);
    }
    // S16: fragments of k-step h (32 elements of K, h < 2): 16-row block mi of A (< 2 * MB), ni of B (< 4)
    __device__ __forceinline__ uint4 rd_a16(const unsigned char* slotA, int h, int mi) const {
        return *reinterpret_cast<const uint4*>(slotA + a_row + mi * 2048 + fco[h]);
    }
    __device__ __forceinline__ uint4 rd_b16(const unsigned char* slotB, int h, int ni) const {
        return *reinterpret_cast<const uint4*>(slotB + b_row + ni * 2048 + fco[h]);
    }
    // k-step 0 of a slab into the fragment registers a step starts from
    __device__ __forceinline__ void first_fragments(uint4 (&fa)[MB], uint4 (&fb)[2][2], const unsigned char* slotA,
                                                    const unsigned char* slotB) const {
        if constexpr (S16) {
#pragma unroll
            for (int mi = 0; mi < MB; ++mi) fa[mi] = rd_a16(slotA, 0, mi);
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) fb[ni >> 1][ni & 1] = rd_b16(slotB, 0, ni);
        } else {
#pragma unroll
            for (int mi = 0; mi < MB; ++mi) fa[mi] = rd_a(slotA, 0, mi);
            fb[0][0] = rd_b(slotB, 0, 0);
            fb[0][1] = rd_b(slotB, 0, 1);
        }
    }
    // head of a slab stream: slab 0 entirely, then the A pieces of slab 1 (its B pieces ride on step 0's first k-step)
    template <class Src>
    __device__ __forceinline__ void prologue(const __amdgpu_buffer_rsrc_t& rsA, const __amdgpu_buffer_rsrc_t& rsB, unsigned char* a0,
                                             unsigned char* b0, unsigned char* a1, unsigned char* b1, const Src& src) const {
#pragma unroll
        for (int j = 0; j < NPIECE; ++j) issue_piece(0, *this, rsA, rsB, a0, b0, 0, j, src);
        __builtin_amdgcn_s_waitcnt(0x0F70);
        __builtin_amdgcn_s_barrier();
#pragma unroll
        for (int j = 0; j < MB; ++j) issue_piece(0, *this, rsA, rsB, a1, b1, 1, j, src);
    }
};

// LP = 2, full-line step: the software pipeline of run_pipelined64 on four 16-element k-steps per slab.  Slab kt in cur (visible),
// slab kt+1 arriving in nxt; fa / fb[0] hold k-step 0 of slab kt.  The barrier of slab kt+1 sits before the LAST k-step of slab kt
// (every read of slab kt has been issued by then); the A pieces of slab kt+2 go out behind the MFMA pairs of that last k-step
// (into the slot the barrier freed), the B pieces of slab kt+1 behind those of the first k-step.  One slab of prefetch distance
// (the slot it lands in is read until the barrier), so the wait before the barrier is vmcnt(0).
template <class OP, int MB, bool SPLIT, class Src>
__device__ __forceinline__ void step_full_line(f32x16 (&acc)[MB][2], uint4 (&fa)[MB], uint4 (&fb)[2][2], const Ring128<MB, SPLIT>& g,
                                               const __amdgpu_buffer_rsrc_t& rsA, const __amdgpu_buffer_rsrc_t& rsB, int kt,
                                               unsigned char* curA, unsigned char* curB, unsigned char* nxtA, unsigned char* nxtB,
                                               const Src& src) {
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        if (h == 3) {
            __builtin_amdgcn_s_waitcnt(0x0F70);
            __builtin_amdgcn_s_barrier();
            pin();
        }
#pragma unroll
        for (int mi = 0; mi < MB; ++mi) {
            mfma_pair<OP>(acc[mi], fa[mi], fb[h & 1]);
            pin();
            // (fco[] indices kept in range: an out-of-bounds index in a dead arm defeats SROA)
            fa[mi] = h < 3 ? g.rd_a(curA, h < 3 ? h + 1 : 0, mi) : g.rd_a(nxtA, 0, mi);
            if (mi == 1) {
                fb[(h + 1) & 1][0] = h < 3 ? g.rd_b(curB, h < 3 ? h + 1 : 0, 0) : g.rd_b(nxtB, 0, 0);
                fb[(h + 1) & 1][1] = h < 3 ? g.rd_b(curB, h < 3 ? h + 1 : 0, 1) : g.rd_b(nxtB, 0, 1);
            }
            if (h == 3) issue_piece(0, g, rsA, rsB, curA, curB, kt + 2, mi, src);
            if (h == 0) {
#pragma unroll
                for (int jb = mi; jb < 4; jb += MB) issue_piece(0, g, rsA, rsB, nxtA, nxtB, kt + 1, MB + jb, src);
            }
            pin();
        }
    }
}

// S16: the same walk in four QUARTERS of MB groups, quarter q = k-step q >> 1, A fragments (q & 1) * MB + mi
template <class OP, int MB, bool SPLIT, class Src>
__device__ __forceinline__ void step_full_line(f32x16 (&acc)[MB][2], uint4 (&fa)[MB], uint4 (&fb)[2][2],
                                               const Ring128<MB, SPLIT, true>& g, const __amdgpu_buffer_rsrc_t& rsA,
                                               const __amdgpu_buffer_rsrc_t& rsB, int kt, unsigned char* curA, unsigned char* curB,
                                               unsigned char* nxtA, unsigned char* nxtB, const Src& src) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (q == 3) {
            __builtin_amdgcn_s_waitcnt(0x0F70);
            __builtin_amdgcn_s_barrier();
            pin();
        }
#pragma unroll
        for (int mi = 0; mi < MB; ++mi) {
            mfma_quad<OP>(acc, (q & 1) * MB + mi, fa[mi], fb[0], fb[1]);
            pin();
            // the fragment this register holds a quarter from now
            fa[mi] = q == 0 ? g.rd_a16(curA, 0, MB + mi)
                   : q == 1 ? g.rd_a16(curA, 1, mi)
                   : q == 2 ? g.rd_a16(curA, 1, MB + mi)
                            : g.rd_a16(nxtA, 0, mi);
            if ((q & 1) && mi == MB - 1) {
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) fb[ni >> 1][ni & 1] = q == 1 ? g.rd_b16(curB, 1, ni) : g.rd_b16(nxtB, 0, ni);
            }
            if (q == 3) issue_piece(0, g, rsA, rsB, curA, curB, kt + 2, mi, src);
            if (q == 0) {
#pragma unroll
                for (int jb = mi; jb < 4; jb += MB) issue_piece(0, g, rsA, rsB, nxtA, nxtB, kt + 1, MB + jb, src);
            }
            pin();
        }
    }
}

template <int MB>
__device__ __forceinline__ void zero(f32x16 (&acc)[MB][2]) {
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
}

}  // namespace kloop

// ---------------------------------------------------------------------------------------------------
// The drivers: prologue issues, the ring-unrolled loop, the tails.  MACROS, expanded in the kernel's own scope, around the step
// templates above: written as one more level of function template, hipcc no longer folds the liveness test of a piece that the
// loop's own bound decides (slab kt+1 is always live inside the full-line loop) -- a select and a register per piece, 4 to 10
// VGPRs on kernels that sit at 235 - 256.  OP: kloop::Bf16 / kloop::F16; G: the Ring64 / Ring128 object; R0..: the slot objects;
// NK: slabs of K (64-byte ones, rounded up, for the first two; whole 128-byte ones for the third); ISSUE / SRC: the functor.
// ---------------------------------------------------------------------------------------------------
#define KLOOP_RUN_FETCH_AFTER_BARRIER(OP, ACC, G, R0, R1, R2, R3, NK, ISSUE)                                 \
    do {                                                                                                   \
        ISSUE(0, R0);                                                                                      \
        ISSUE(1, R1);                                                                                      \
        ISSUE(2, R2);                                                                                      \
        int kl_kt = 0;                                                                                     \
        for (; kl_kt + 4 <= (NK); kl_kt += 4) {                                                            \
            kloop::step_fetch_after_barrier<OP>(ACC, G, kl_kt, R0, R3, ISSUE);                             \
            kloop::step_fetch_after_barrier<OP>(ACC, G, kl_kt + 1, R1, R0, ISSUE);                         \
            kloop::step_fetch_after_barrier<OP>(ACC, G, kl_kt + 2, R2, R1, ISSUE);                         \
            kloop::step_fetch_after_barrier<OP>(ACC, G, kl_kt + 3, R3, R2, ISSUE);                         \
        }                                                                                                  \
        kloop::keep_whole_if_s16<OP>(ACC);                                                                 \
        if (kl_kt < (NK)) kloop::step_fetch_after_barrier<OP>(ACC, G, kl_kt, R0, R3, ISSUE);               \
        if (kl_kt + 1 < (NK)) kloop::step_fetch_after_barrier<OP>(ACC, G, kl_kt + 1, R1, R0, ISSUE);       \
        if (kl_kt + 2 < (NK)) kloop::step_fetch_after_barrier<OP>(ACC, G, kl_kt + 2, R2, R1, ISSUE);       \
        kloop::keep_whole_if_s16<OP>(ACC);                                                                 \
    } while (0)

#define KLOOP_RUN_PIPELINED64(OP, MB, ACC, G, RSA, RSB, R0, R1, R2, R3, NK, SRC)                           \
    do {                                                                                                   \
        uint4 kl_fa[MB], kl_fb0[2], kl_fb1[2];                                                             \
        kloop::prologue_pipelined64(kl_fa, kl_fb0, kl_fb1, G, RSA, RSB, R0, R1, R2, R3, SRC);                      \
        int kl_kt = 0;                                                                                     \
        for (; kl_kt + 4 <= (NK); kl_kt += 4) {                                                            \
            kloop::step_pipelined64<OP>(ACC, kl_fa, kl_fb0, kl_fb1, G, RSA, RSB, kl_kt, R0, R1, SRC);      \
            kloop::step_pipelined64<OP>(ACC, kl_fa, kl_fb0, kl_fb1, G, RSA, RSB, kl_kt + 1, R1, R2, SRC);  \
            kloop::step_pipelined64<OP>(ACC, kl_fa, kl_fb0, kl_fb1, G, RSA, RSB, kl_kt + 2, R2, R3, SRC);  \
            kloop::step_pipelined64<OP>(ACC, kl_fa, kl_fb0, kl_fb1, G, RSA, RSB, kl_kt + 3, R3, R0, SRC);  \
        }                                                                                                  \
        kloop::keep_whole_if_s16<OP>(ACC);                                                                 \
        if (kl_kt < (NK)) kloop::step_pipelined64<OP>(ACC, kl_fa, kl_fb0, kl_fb1, G, RSA, RSB, kl_kt, R0, R1, SRC);         \
        if (kl_kt + 1 < (NK)) kloop::step_pipelined64<OP>(ACC, kl_fa, kl_fb0, kl_fb1, G, RSA, RSB, kl_kt + 1, R1, R2, SRC); \
        if (kl_kt + 2 < (NK)) kloop::step_pipelined64<OP>(ACC, kl_fa, kl_fb0, kl_fb1, G, RSA, RSB, kl_kt + 2, R2, R3, SRC); \
        kloop::keep_whole_if_s16<OP>(ACC);                                                                 \
    } while (0)

#define KLOOP_RUN_FULL_LINE(OP, MB, ACC, G, RSA, RSB, R0, R1, NK2, SRC)                                    \
    do {                                                                                                   \
        uint4 kl_fa[MB], kl_fb[2][2];                                                                      \
        (G).prologue(RSA, RSB, R0, R0, R1, R1, SRC);                                                       \
        (G).first_fragments(kl_fa, kl_fb, R0, R0);                                                         \
        int kl_kt = 0;                                                                                     \
        for (; kl_kt + 2 <= (NK2); kl_kt += 2) {                                                           \
            kloop::step_full_line<OP>(ACC, kl_fa, kl_fb, G, RSA, RSB, kl_kt, R0, R0, R1, R1, SRC);         \
            kloop::step_full_line<OP>(ACC, kl_fa, kl_fb, G, RSA, RSB, kl_kt + 1, R1, R1, R0, R0, SRC);     \
        }                                                                                                  \
        kloop::keep_whole_if_s16<OP>(ACC);                                                                 \
        if (kl_kt < (NK2)) kloop::step_full_line<OP>(ACC, kl_fa, kl_fb, G, RSA, RSB, kl_kt, R0, R0, R1, R1, SRC); \
        kloop::keep_whole_if_s16<OP>(ACC);                                                                 \
    } while (0)
