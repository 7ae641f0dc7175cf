// The tiled bf16 family (index of the GEMM files: gemm.hip): ONE 512-thread workgroup per CU on a (64*MB) x 256 tile.
//   gemm_kernel_v7   template parameter LP = K-loop form: 0 barrier-then-fetch (patch gather, K tails), 1 software-pipelined
//                    64-byte slabs, 2 full-line 128-byte slabs; its residual instances of the full-line form park the residual
//                    rows in LDS (ResidParkSrc, -DPV_GEMM_RESID_PARK)
//   gemm_kernel_v8   v7's full-line form made persistent: a workgroup walks its tiles, their K slabs one stream
// The K loops -- slot geometry, swizzles, step bodies, drivers -- and the XCD-aware tile order live in kloop.hpp, shared with the SAE
// filter GEMM (sae_enc_gemm.hip); the kernels here keep their LDS objects, descriptors, piece sources and epilogues.
// Compiled as part of gemm.hip, which includes it once, beside gemm_v4.hpp (whose head says why the two share a translation unit).
#pragma once
#include "gemm_epi.hpp"

#include <hip/hip_ext.h>

namespace {

// ---------------------------------------------------------------------------------------------------
// v7 mainloop: ONE 512-thread workgroup per CU, (64*MB) x 256 tile (MB = 4: 256 x 256, MB = 5: 320 x 256).
//   The 128 x 128 tiles of v4 pull 1/64 byte of operand per flop out of L2: 68 GB per bs=512 B/32 forward,
//   ~15 TB/s sustained at v4's speed -- the L2 -> LDS path, not the matrix pipe, is what v4 saturates
//   (profiles/r01_notes.md).  Here the byte/flop ratio is 1/128 (MB = 4) or 1/142 (MB = 5):
//     * 8 waves as 2 (M) x 4 (N); a wave owns (32*MB) x 64 outputs (14 ds_read_b128 per 20 MFMAs at MB = 5)
//     * slot = (64*MB + 256) rows x 64 B (36 KB at MB = 5); FOUR slots (144 KB of the 160 KB) -> slab k+3 is
//       issued while slab k is multiplied, three slabs (108 KB per CU) in flight
//     * per slab a wave issues NA = ceil(4*MB / 8) A-instructions + 2 B-instructions; at MB = 5 waves 4..7 have
//       only 2 real A pieces -- their third is an out-of-range (zero-fill) DMA into a pad, so that every
//       wave retires the same number and the counted wait stays a compile-time vmcnt(2 * (NA + 2))
//     * MB = 5 makes M = 25600 (512 images x 50 tokens) exactly 80 row tiles: the N = 768 GEMMs (O-projection,
//       MLP-2) are 240 tiles = ONE round of the 256 CUs, the QKV GEMM 720 = three
// ---------------------------------------------------------------------------------------------------
// The RESIDUAL PARK of the full-line form (LP = 2, EPI = RESID; -DPV_GEMM_RESID_PARK=0 builds the form without it).  The store
// epilogue used to load the residual rows of blocks 1 .. MB-1 behind the stores of the block before; vmcnt retires in issue order,
// so every wait for a row was a wait for two store streams to leave the CU while 240 CUs stored at once.  The full-line loop
// already issues 3 * MB + 4 DEAD pieces per wave off its end (the A and B pieces of slab nk2, the A pieces of slab nk2 + 1), counted
// in its waits; here those pieces fetch this wave's residual chunks instead -- for (block mi >= 1, pass it) lane l the 16 bytes it
// would have loaded into e_res[mi][it] -- into ring slots the loop has freed, 1 KiB per piece, lane l at byte 16 l.  The epilogue
// reads its chunk back with one ds_read_b128 from where the same lane's DMA put it and contains no load at all.
//   park piece i = (mi - 1) * 4 + it, NPARK = 4 * (MB - 1) per wave.  Slab nk2 would have gone to slot P = nk2 & 1, which is free
//   from the barrier of step nk2 - 2 on: its MB + 4 dead pieces per wave (8 waves x (MB + 4) KiB = the whole slot) take park pieces
//   0 .. MB + 3 at  (wave * NP0 + i) KiB.  The A pieces of slab nk2 + 1 go out behind the LAST barrier of the loop into the other
//   slot, free from there on: park pieces NP0 .. at  (wave * NP1 + i - NP0) KiB, and the 2 * MB - 8 that are left (two at MB = 5,
//   none at MB = 4) are issued directly behind the loop, in front of the first store.  K of one or two slabs needs nothing else: the
//   prologue's A pieces of slab 1 are the dead pieces of slab nk2 when nk2 = 1 and go through the same functor.
//   Only the issuing wave reads a parked piece, behind its own vmcnt(0): no barrier.  The fp32 transposition leaves the ring for
//   2 KB per wave beside it (8 rows per pass, as gemm_kernel_v8): 2 * 72 + 16 KB = the CU's 160 KB at MB = 5.
//   The source is a descriptor over THIS WAVE's rows and columns of the residual (base at its first row / column, range ending
//   with its last real row's last real column): rows >= M zero-fill; a chunk at columns >= N of a row that is not the last reads
//   bytes of the residual buffer between that row and the next, and is never used (e_rows_left = 0 for such a lane).
//   resid may be out1 (the plan never does that: vit_plan.hip adds resid_pre into resid_mid and resid_mid into resid_post, three
//   buffers): a tile parks only rows and columns that it alone stores, and all of them before its first store.
#ifndef PV_GEMM_RESID_PARK
#define PV_GEMM_RESID_PARK 1
#endif
template <int MB, class R128>
struct ResidParkSrc {
    static constexpr int NPARK = 4 * (MB - 1), NP0 = MB + 4, NP1 = NPARK - NP0, NLOOP = NP0 + MB;   // NLOOP .. NPARK-1: behind the loop
    static_assert(NP0 * 8 * 1024 == R128::SLOT && NP1 >= 0 && NP1 * 8 * 1024 <= R128::SLOT && NLOOP <= NPARK, "park geometry");
    __amdgpu_buffer_rsrc_t rsR;
    unsigned pA0, pB0, strideA, strideB, lpR, ldrB;
    int nk2, wave;
    // uniform source term / destination (bytes into its slot) of park piece i
    __device__ static __forceinline__ constexpr int park_row(int i) { return (1 + (i >> 2)) * 32 + epi_pass_row<S16>(i & 3); }
    __device__ __forceinline__ unsigned park_u(int i) const { return (unsigned)park_row(i) * ldrB; }
    __device__ __forceinline__ int park_dst(int i) const { return i < NP0 ? (wave * NP0 + i) * 1024 : (wave * NP1 + (i - NP0)) * 1024; }
    // piece j of slab kt into the slot: the operand piece, or off the end of K (every condition uniform, selects only) park piece
    // j of slab nk2's MB + 4, NP0 + j of slab nk2 + 1's MB
    __device__ __forceinline__ void piece(const R128& g, const __amdgpu_buffer_rsrc_t& rsA, const __amdgpu_buffer_rsrc_t& rsB,
                                          unsigned char* slotA, unsigned char* slotB, int kt, int j) const {
        const bool dead = kt >= nk2, second = kt > nk2;
        // (the row constant and the wave's base are selected, then scaled: products selected instead are one loop-invariant scalar
        // register per piece, and the MB = 4 instance runs out of them)
        const int i1 = NP0 + j < NPARK ? NP0 + j : NPARK - 1;      // (in range where it is not used: B pieces are never `second`)
        const unsigned pu = (unsigned)(second ? park_row(i1) : park_row(j)) * ldrB;
        const int pd = ((second ? wave * NP1 : wave * NP0) + j) * 1024;
        const unsigned kbase = (unsigned)kt * 128u;
        if (j < MB) {
            const unsigned off = (dead ? lpR : pA0) + (dead ? pu : (unsigned)j * strideA + kbase);
            kloop::dma16(dead ? rsR : rsA, slotA + (dead ? pd : (j * 8 + wave) * 1024), off);
        } else {
            const unsigned off = (dead ? lpR : pB0) + (dead ? pu : (unsigned)(j - MB) * strideB + kbase);
            kloop::dma16(dead ? rsR : rsB, slotB + (dead ? pd : R128::B_BASE + ((j - MB) * 8 + wave) * 1024), off);
        }
    }
};

template <typename T, int MB, int EPI, int ACT, int LP = 0>
__global__ __launch_bounds__(512, 2) void gemm_kernel_v7(const GemmParams p) {
    static_assert(sizeof(T) == 2, "v7 is the bf16 kernel");
    using R64 = kloop::Ring64<MB, S16>;
    using R128 = kloop::Ring128<MB, false, S16>;
    constexpr int TM = 64 * MB, TN = 256, SLOT = R64::SLOT, NA = R64::NA;
    static_assert(R128::SLOT == 2 * SLOT, "a full-line slot is two 64-byte-slab slots");
    constexpr bool PARK = PV_GEMM_RESID_PARK && LP == 2 && EPI == PV_EPI_RESID;
    using Park = ResidParkSrc<MB, R128>;
    __shared__ __attribute__((aligned(16))) unsigned char stage[PARK ? 8 * 2048 : 16];      // (PARK: the epilogue's transposition)
    static_assert(!PARK || 4 * SLOT + 8 * 2048 <= 160 * 1024, "one workgroup per CU");
    // the ring slots, one object each (kloop.hpp).  LP >= 2 (full-line form): two slots of 128-byte rows in ring0 / ring1, the other
    // objects shrink to stubs
    __shared__ __attribute__((aligned(16))) unsigned char ring0[LP >= 2 ? 2 * SLOT : SLOT];
    __shared__ __attribute__((aligned(16))) unsigned char ring1[LP >= 2 ? 2 * SLOT : SLOT];
    __shared__ __attribute__((aligned(16))) unsigned char ring2[LP >= 2 ? 16 : SLOT];
    __shared__ __attribute__((aligned(16))) unsigned char ring3[LP >= 2 ? 16 : SLOT];
    __shared__ __attribute__((aligned(16))) unsigned char pad[LP < 2 ? R64::PAD_BYTES : 16];
    constexpr int EB = DT<T>::kBytes;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int bid = blockIdx.x;
    const int swz = kloop::xcd_run(bid, gridDim.x);
    int tile_m, tile_n;
    kloop::TileOrder<TM, TN>(p.M, p.N).at(swz, tile_m, tile_n);
    const int m0 = tile_m * TM, n0 = tile_n * TN;
    trace_stamp(p.trace, bid, 0);

    const unsigned Kb = (unsigned)p.K * EB;
    // PATCH A operand (patch size 32, bf16): the 64 bytes of K that slab kt covers are ONE contiguous run of the
    // NCHW image -- channel kt / 32, patch row kt % 32 -- so the im2col-free gather is only a different row base and
    // slab offset for the same DMA (patch_embedding.py:26-32)
    const bool patch = p.a_mode == PV_A_PATCH;
    const unsigned a_span = patch ? (unsigned)(p.M / (p.pG * p.pG)) * (unsigned)p.pC * (unsigned)p.pS * (unsigned)p.pS * EB
                                  : (unsigned)p.M * (unsigned)p.lda * EB;
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.A), 0, (int)a_span, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<void*>(p.Bt), 0, (int)((unsigned)p.N * (unsigned)p.ldb * EB), 0x00020000);      // (rows >= N: past the range -> 0)
    const unsigned ldaB = (unsigned)p.lda * EB, ldbB = (unsigned)p.ldb * EB;

    f32x16 acc[MB][2];
    kloop::zero(acc);
    const int l31 = lane & 31, half = lane >> 5;

    // epilogue operands in flight before the K loop (see v4): bias chunk + residual rows of block 0.
    // The launcher guarantees vec_out and N % 8 == 0: whole 8-element chunks only.
    const int e_gn = n0 + wn * 64 + (lane & 7) * 8;
    const bool e_live = e_gn < p.N;
    const int e_lrow = epi_lane_row<S16>(lane);
    const int e_rows_left = e_live ? p.M - (m0 + wm * 32 * MB + e_lrow) : 0;    // row mi*32 + pass_row(it) of this lane is real iff < e_rows_left
    uint4 e_bias = make_uint4(0, 0, 0, 0);
    constexpr int NRES = EPI == PV_EPI_RESID && !PARK ? MB : 1;      // (PARK: block 0 in registers, the others in LDS)
    uint4 e_res[NRES][4];
#pragma unroll
    for (int mi = 0; mi < NRES; ++mi)
#pragma unroll
        for (int it = 0; it < 4; ++it) e_res[mi][it] = make_uint4(0, 0, 0, 0);
    int e_col = e_gn;
    T* e_out0 = reinterpret_cast<T*>(p.out0);
    const T* e_rbase = reinterpret_cast<const T*>(p.resid) + (int64_t)(m0 + wm * 32 * MB + e_lrow) * p.ldr + e_gn;
#define PV_V7_FETCH_RES(MI)                                                                          \
    if constexpr (EPI == PV_EPI_RESID) {                                                             \
        _Pragma("unroll") for (int it = 0; it < 4; ++it)                                             \
            if ((MI) * 32 + epi_pass_row<S16>(it) < e_rows_left)                                     \
                e_res[MI][it] = *reinterpret_cast<const uint4*>(e_rbase + (int64_t)((MI) * 32 + epi_pass_row<S16>(it)) * p.ldr); \
    }
    if (e_live) {
        const T* bias = reinterpret_cast<const T*>(p.bias0);
        if constexpr (EPI == PV_EPI_QKV) {
            const int which = e_gn / p.nsplit;
            e_col = e_gn - which * p.nsplit;
            if (which == 1) { e_out0 = reinterpret_cast<T*>(p.out1); bias = reinterpret_cast<const T*>(p.bias1); }
            if (which == 2) { e_out0 = reinterpret_cast<T*>(p.out2); bias = reinterpret_cast<const T*>(p.bias2); }
        }
        if (bias) e_bias = *reinterpret_cast<const uint4*>(bias + e_col);
    }
    PV_V7_FETCH_RES(0)

    // the K loop (kloop.hpp); what is written here is where each form's pieces come from
    if constexpr (LP == 0) {
        // any A operand, any K: per piece a per-lane base, a uniform slab term and the K-tail test
        const R64 g(lane, wave, pad);
        const int nk = (int)((Kb + 63) / 64);
        const bool ktail = (Kb % 64) != 0;
        unsigned offA[NA], kcA[NA], offB[2], kcB[2];
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            const int row = g.piece_row(lane, j);
            kcA[j] = R64::piece_col(lane, row);
            if (patch) {
                const int gm = m0 + row, np = p.pG * p.pG;
                const int b = gm / np, pidx = gm - b * np;
                const int py = pidx / p.pG, px = pidx - py * p.pG;
                offA[j] = (unsigned)(((b * p.pC) * p.pS + py * p.pP) * p.pS + px * p.pP) * EB + kcA[j];      // image b >= B: past the range -> 0
            } else {
                offA[j] = (unsigned)(m0 + row) * ldaB + kcA[j];
            }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int row = g.piece_row(lane, j);
            kcB[j] = R64::piece_col(lane, row);
            offB[j] = (unsigned)(n0 + row) * ldbB + kcB[j];
        }
        auto issue = [&](int kt, unsigned char* slot) {
            const unsigned kbase = (unsigned)kt * 64;
            bool dead = (kt >= nk);
#ifdef PV_TUNING
            dead |= (((p.dbg & 1) != 0) & (kt >= 3));
#endif
            const unsigned kbaseA = patch ? (unsigned)((kt >> 5) * p.pS * p.pS + (kt & 31) * p.pS) * EB : kbase;
#pragma unroll
            for (int j = 0; j < NA; ++j)
                g.issue(rsA, rsB, slot, j, (dead | !g.real_a(j) | (ktail & (kbase + kcA[j] >= Kb))) ? kloop::DEAD : offA[j] + kbaseA);
#pragma unroll
            for (int j = 0; j < 2; ++j)
                g.issue(rsA, rsB, slot, NA + j, (dead | (ktail & (kbase + kcB[j] >= Kb))) ? kloop::DEAD : offB[j] + kbase);
        };
        KLOOP_RUN_FETCH_AFTER_BARRIER(kloop::Bf16, acc, g, ring0, ring1, ring2, ring3, nk, issue);
    } else if constexpr (LP == 1) {
        // plain A operand, whole 64-byte slabs only (the launcher keeps LP = 0 for the patch gather and for a K tail): a piece's
        // source offset is one per-lane base + a uniform term, two VALU per piece
        const R64 g(lane, wave, pad);
        const int nk = (int)((Kb + 63) / 64);
        const int row0 = g.piece_row(lane, 0);
        const unsigned pA0 = (unsigned)(m0 + row0) * ldaB + R64::piece_col(lane, row0);
        const unsigned pB0 = (unsigned)(n0 + row0) * ldbB + R64::piece_col(lane, row0);
        const unsigned strideA = R64::PIECE_STRIDE * ldaB, strideB = R64::PIECE_STRIDE * ldbB;
        auto src = [&](int kt, int j) -> unsigned {
            const unsigned kbase = (unsigned)kt * 64;
            const bool dead = (kt >= nk);
            if (j < NA) return (dead | !g.real_a(j)) ? kloop::DEAD : pA0 + ((unsigned)j * strideA + kbase);
            return dead ? kloop::DEAD : pB0 + ((unsigned)(j - NA) * strideB + kbase);
        };
        KLOOP_RUN_PIPELINED64(kloop::Bf16, MB, acc, g, rsA, rsB, ring0, ring1, ring2, ring3, nk, src);
    } else {
        // plain A operand, whole 128-byte slabs only
        const R128 g(lane, wave);
        const int nk2 = (int)(Kb / 128);
        const unsigned pA0 = (unsigned)(m0 + g.piece_row(lane)) * ldaB + g.piece_col(lane);
        const unsigned pB0 = (unsigned)(n0 + g.piece_row(lane)) * ldbB + g.piece_col(lane);
        const unsigned strideA = R128::PIECE_STRIDE * ldaB, strideB = R128::PIECE_STRIDE * ldbB;
        auto src = [&](int kt, int j) -> unsigned {
            const unsigned kbase = (unsigned)kt * 128;
            const bool dead = (kt >= nk2);
            if (j < MB) return dead ? kloop::DEAD : pA0 + ((unsigned)j * strideA + kbase);
            return dead ? kloop::DEAD : pB0 + ((unsigned)(j - MB) * strideB + kbase);
        };
        if constexpr (PARK) {
            // the same pieces, and off the end of K the residual park (see ResidParkSrc)
            (void)src;
            const int r_row0 = m0 + wm * 32 * MB, r_col0 = n0 + wn * 64;
            const int r_rows = min(max(p.M - r_row0, 0), 32 * MB), r_cols = min(max(p.N - r_col0, 0), 64);
            const unsigned ldrB = (unsigned)p.ldr * EB;
            const unsigned r_bytes = (r_rows > 0 && r_cols > 0) ? (unsigned)(r_rows - 1) * ldrB + (unsigned)r_cols * EB : 0u;
            const unsigned char* r_base = reinterpret_cast<const unsigned char*>(p.resid) + ((int64_t)r_row0 * p.ldr + r_col0) * EB;
            const Park park{__builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(r_base), 0, (int)r_bytes, 0x00020000),
                            pA0, pB0, strideA, strideB, (unsigned)e_lrow * ldrB + (unsigned)(lane & 7) * 16u, ldrB, nk2, wave};
            KLOOP_RUN_FULL_LINE(kloop::Bf16, MB, acc, g, rsA, rsB, ring0, ring1, nk2, park);
            // what the loop's dead pieces did not take, into the slot its last barrier freed
            unsigned char* const slot1 = (nk2 & 1) ? ring0 : ring1;
#pragma unroll
            for (int i = Park::NLOOP; i < Park::NPARK; ++i) kloop::dma16(park.rsR, slot1 + park.park_dst(i), park.lpR + park.park_u(i));
        } else {
            KLOOP_RUN_FULL_LINE(kloop::Bf16, MB, acc, g, rsA, rsB, ring0, ring1, nk2, src);
        }
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);     // vmcnt(0): drain the off-the-end prefetches (PARK: this wave's parked rows have landed)
    if constexpr (!PARK) __syncthreads();   // (PARK: the epilogue touches nothing another wave reads or writes)
    trace_stamp(p.trace, bid, 1);
#ifdef PV_TUNING
    if (p.dbg & 2) {
        if (acc[0][0][0] == 123.456f) reinterpret_cast<float*>(p.out0)[0] = acc[1][1][3] + acc[0][1][2] + acc[1][0][1];
        return;
    }
#endif

    constexpr int CLD = 64;
    [[maybe_unused]] float* Cs = reinterpret_cast<float*>((wave < 4 ? ring0 : ring1) + (wave & 3) * (32 * CLD * 4));
    const pv_f32x2 e_b[4] = {unpack2(e_bias.x), unpack2(e_bias.y), unpack2(e_bias.z), unpack2(e_bias.w)};
    const int64_t e_row0 = (int64_t)(m0 + wm * 32 * MB + e_lrow) * p.ldo;
    T* const o0_base = e_out0 ? e_out0 + e_row0 + e_col : nullptr;
    T* const o1_base = reinterpret_cast<T*>(p.out1) + e_row0 + e_gn;
    [[maybe_unused]] const float* Cr = Cs + epi_read_off<S16>(lane);
    if constexpr (PARK) {
        // a store stream with no load in it: 8 rows x 64 columns per pass through the wave's own 2 KB (the ring holds the parked
        // rows), the residual chunk of blocks >= 1 from where this lane's DMA put it
        float* const Cs8 = reinterpret_cast<float*>(stage + wave * 2048);
        const float* const Cr8 = Cs8 + epi_read_off<S16>(lane);
        [[maybe_unused]] float* const Cw8 = Cs8 + half * 256 + l31;
        const unsigned char* const slot0 = (Kb / 128 & 1) ? ring1 : ring0;
        const unsigned char* const slot1 = (Kb / 128 & 1) ? ring0 : ring1;
        const unsigned char* const pk0 = slot0 + (wave * Park::NP0) * 1024 + lane * 16;
        const unsigned char* const pk1 = slot1 + (wave * Park::NP1) * 1024 + lane * 16;
#pragma unroll
        for (int mi = 0; mi < MB; ++mi) {
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                if constexpr (S16) {
                    stage_pass16(Cs8, acc[mi], it, lane);
                } else {
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                        for (int j = 0; j < 4; ++j) Cw8[j * 64 + ni * 32] = acc[mi][ni][4 * it + j];
                }
                __builtin_amdgcn_wave_barrier();
                if (mi * 32 + epi_pass_row<S16>(it) < e_rows_left) {
                    const float4 x0 = *reinterpret_cast<const float4*>(Cr8);
                    const float4 x1 = *reinterpret_cast<const float4*>(Cr8 + 4);
                    const int i = mi > 0 ? (mi - 1) * 4 + it : 0;
                    const uint4 res = mi == 0 ? e_res[0][it]
                                              : *reinterpret_cast<const uint4*>(i < Park::NP0 ? pk0 + i * 1024 : pk1 + (i - Park::NP0) * 1024);
                    const int64_t ro = (int64_t)(mi * 32 + epi_pass_row<S16>(it)) * p.ldo;
                    epi8_bf16<EPI, ACT>(x0, x1, e_b, o0_base ? o0_base + ro : nullptr, o1_base + ro, res);
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
    } else {
#pragma unroll
    for (int mi = 0; mi < MB; ++mi) {
        if constexpr (S16) {
#pragma unroll
            for (int it = 0; it < 4; ++it) stage_pass16(Cs + it * 8 * CLD, acc[mi], it, lane);
        } else {
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int row = (e & 3) + 8 * (e >> 2) + 4 * half;
                    Cs[row * CLD + ni * 32 + l31] = acc[mi][ni][e];
                }
        }
        __builtin_amdgcn_wave_barrier();
        // residual rows two blocks ahead: staging block mi freed 32 accumulator registers, which now carry the
        // rows of blocks 2mi+1 and 2mi+2 -- from block 2 on a load has two blocks of stores to land behind
        // (indices kept in range: an OOB index in a dead arm defeats SROA)
        if (2 * mi + 1 < MB) { PV_V7_FETCH_RES((2 * mi + 1 < MB ? 2 * mi + 1 : 0)) }
        if (2 * mi + 2 < MB) { PV_V7_FETCH_RES((2 * mi + 2 < MB ? 2 * mi + 2 : 0)) }
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            if (mi * 32 + epi_pass_row<S16>(it) < e_rows_left) {
                const float4 x0 = *reinterpret_cast<const float4*>(Cr + it * 8 * CLD);
                const float4 x1 = *reinterpret_cast<const float4*>(Cr + it * 8 * CLD + 4);
                const int64_t ro = (int64_t)(mi * 32 + epi_pass_row<S16>(it)) * p.ldo;
                epi8_bf16<EPI, ACT>(x0, x1, e_b, o0_base ? o0_base + ro : nullptr, o1_base + ro,
                                    e_res[EPI == PV_EPI_RESID ? mi : 0][it]);
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    }
#undef PV_V7_FETCH_RES
    trace_stamp(p.trace, bid, 2);
}

// ---------------------------------------------------------------------------------------------------
// v8: the v7 full-line kernel made PERSISTENT.  One 512-thread workgroup per CU walks its tiles (virtual block ids bid,
// bid + grid, ...: the same XCD-aware tile order as v7) and the K slabs of consecutive tiles form ONE stream through the
// two-slot ring: the prefetches v7 issues off the end of its K loop (dead DMAs there) are the NEXT tile's first slab and the
// A pieces of its second, so a tile's store epilogue runs with the next tile's operands already in LDS / in flight, the
// next K loop starts without a launch, a DMA prologue or a drained store queue in front of it, and the workgroups of a
// launch drift apart instead of computing together and then storing together (profiles/r02_gemm_phase_trace.txt).
//   * what changes against v7 LP == 2: the epilogue's transposition no longer borrows the ring (it holds the next tile's
//     slab): 2 KB per wave of dedicated LDS (the 16 KB the two 72 KB slots leave), 8 rows per pass instead of 32;
//     no workgroup barrier and no vmcnt(0) between K loop and epilogue; slab indices past the tile's end address the next
//     tile (selects on a uniform condition: no branch around an LDS-DMA)
//   * the MFMA / fragment-read / DMA-issue order inside the K loop is v7's, and so is the k order of every output's fp32 sum:
//     results are bit-identical to v7's
//   * legal where v7's full-line loop is: plain A operand, K a whole EVEN number of 128-byte slabs (the two slots alternate
//     per slab: an odd count would swap their roles from tile to tile)
// ---------------------------------------------------------------------------------------------------
// the lane id, computed where it is asked for (asm volatile: neither hoisted nor merged with an earlier copy) -- what the epilogue of
// the persistent kernel derives its addresses from, so that none of them lives through the K loop
__device__ __forceinline__ int lane_id_here() {
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}

template <typename T, int MB, int EPI, int ACT>
__global__ __launch_bounds__(512, 2) void gemm_kernel_v8(const GemmParams p, const int ntiles, const int stagger) {
    static_assert(sizeof(T) == 2, "v8 is a bf16 kernel");
    using R128 = kloop::Ring128<MB, true, S16>;
    constexpr int TM = 64 * MB;
    constexpr int TN = 256;
    constexpr int A2 = R128::A_BYTES, B2 = R128::B_BYTES;             // one slot: (TM + TN) rows x 128 bytes of K
    constexpr int STAGE = 8 * 2048;                                   // epilogue transposition: 8 rows x 64 fp32 per wave
    static_assert(2 * (A2 + B2) + STAGE <= 160 * 1024, "one workgroup per CU");
    // four LDS objects, the A / B part of either slot (one object per slot, kloop.hpp: the ds_reads of one slot must not be taken
    // to alias the DMA writes in flight to the other)
    __shared__ __attribute__((aligned(16))) unsigned char ringA0[A2];
    __shared__ __attribute__((aligned(16))) unsigned char ringA1[A2];
    __shared__ __attribute__((aligned(16))) unsigned char ringB0[B2];
    __shared__ __attribute__((aligned(16))) unsigned char ringB1[B2];
    __shared__ __attribute__((aligned(16))) unsigned char stage[STAGE];
    constexpr int EB = 2;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    // virtual block id -> tile origin (v7's mapping with the virtual grid size: bid and bid + k * gridDim.x sit on the same XCD)
    const kloop::TileOrder<TM, TN> order(p.M, p.N);
    auto tile_of = [&](int vb, int& m0, int& n0) {
        int tile_m, tile_n;
        order.at(kloop::xcd_run(vb, ntiles), tile_m, tile_n);
        m0 = tile_m * TM;
        n0 = tile_n * TN;
    };
    const unsigned Kb = (unsigned)p.K * EB;
    const int nk2 = (int)(Kb / 128);
    const unsigned ldaB = (unsigned)p.lda * EB, ldbB = (unsigned)p.ldb * EB;
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.A), 0, (int)((unsigned)p.M * ldaB), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.Bt), 0, (int)((unsigned)p.N * ldbB), 0x00020000);

    // DMA pieces: per-lane part of the source offset; the tile's origin and the slab are uniform terms
    const R128 g(lane, wave);
    const unsigned lpA = (unsigned)g.piece_row(lane) * ldaB + g.piece_col(lane);
    const unsigned lpB = (unsigned)g.piece_row(lane) * ldbB + g.piece_col(lane);
    const unsigned strideA = R128::PIECE_STRIDE * ldaB, strideB = R128::PIECE_STRIDE * ldbB;
    unsigned uA, uB, uAn = 0, uBn = 0;                              // this tile's / the next tile's uniform origin terms
    bool dead_n = true;
    // piece j of slab s; s >= nk2: slab s - nk2 of the NEXT tile (selects on a uniform condition)
    auto src = [&](int s, int j) -> unsigned {
        const bool nx = s >= nk2;
        const unsigned sb = (unsigned)(nx ? s - nk2 : s) * 128u;
        const bool dead = nx & dead_n;
        const unsigned o = j < MB ? lpA + ((nx ? uAn : uA) + (unsigned)j * strideA + sb)
                                  : lpB + ((nx ? uBn : uB) + (unsigned)(j - MB) * strideB + sb);
        return dead ? kloop::DEAD : o;
    };

    f32x16 acc[MB][2];
    kloop::zero(acc);
    // the tile's slabs alternate between the slots: even ones in ringA0 / ringB0
#define PV_V8_EVEN(KT)                                \
    if constexpr (S16) kloop::keep_whole(acc);        \
    kloop::step_full_line<kloop::Bf16>(acc, fa, fb, g, rsA, rsB, KT, ringA0, ringB0, ringA1, ringB1, src);
#define PV_V8_ODD(KT)                                 \
    if constexpr (S16) kloop::keep_whole(acc);        \
    kloop::step_full_line<kloop::Bf16>(acc, fa, fb, g, rsA, rsB, KT, ringA1, ringB1, ringA0, ringB0, src);

    int vb = blockIdx.x;
    int m0, n0;
    tile_of(vb, m0, n0);
    uA = (unsigned)m0 * ldaB; uB = (unsigned)n0 * ldbB;
    if (stagger > 0) {
        // (A/B knob: workgroups of a launch start a fraction of a tile apart -- see profiles/r05_notes.md)
        const int k = ((blockIdx.x >> 3) & 3) * stagger;
        for (int i = 0; i < k; ++i) __builtin_amdgcn_s_sleep(127);
    }
    trace_stamp(p.trace, vb, 0);
    // the stream's head: slab 0 of the first tile entirely, the A pieces of its slab 1
    g.prologue(rsA, rsB, ringA0, ringB0, ringA1, ringB1, src);

    for (;;) {
        const int vbn = vb + (int)gridDim.x;
        const bool has_next = vbn < ntiles;
        int m0n = 0, n0n = 0;
        if (has_next) tile_of(vbn, m0n, n0n);
        uAn = (unsigned)m0n * ldaB; uBn = (unsigned)n0n * ldbB;
        dead_n = !has_next;

        // epilogue operands of THIS tile in flight under its K loop (v7): bias chunk + residual rows of block 0.  Only the loaded
        // registers live through the loop; every address is recomputed behind it (the loop body runs at the register limit).
        uint4 e_bias = make_uint4(0, 0, 0, 0);
        constexpr int NRES = EPI == PV_EPI_RESID ? MB : 1;
        uint4 e_res[NRES][4];
#pragma unroll
        for (int mi = 0; mi < NRES; ++mi)
#pragma unroll
            for (int it = 0; it < 4; ++it) e_res[mi][it] = make_uint4(0, 0, 0, 0);
#define PV_V8_EPI_GEOMETRY()                                                                                          \
        const int e_lane = lane_id_here();                                                                            \
        const int e_gn = n0 + wn * 64 + (e_lane & 7) * 8;                                                             \
        const bool e_live = e_gn < p.N;                                                                               \
        const int e_rows_left = e_live ? p.M - (m0 + wm * 32 * MB + epi_lane_row<S16>(e_lane)) : 0;                   \
        int e_col = e_gn;                                                                                             \
        T* e_out0 = reinterpret_cast<T*>(p.out0);                                                                     \
        const T* e_biasp = reinterpret_cast<const T*>(p.bias0);                                                       \
        if constexpr (EPI == PV_EPI_QKV) {                                                                            \
            const int which = e_gn / p.nsplit;                                                                        \
            e_col = e_gn - which * p.nsplit;                                                                          \
            if (which == 1) { e_out0 = reinterpret_cast<T*>(p.out1); e_biasp = reinterpret_cast<const T*>(p.bias1); } \
            if (which == 2) { e_out0 = reinterpret_cast<T*>(p.out2); e_biasp = reinterpret_cast<const T*>(p.bias2); } \
        }                                                                                                             \
        const T* e_rbase = reinterpret_cast<const T*>(p.resid) + (int64_t)(m0 + wm * 32 * MB + epi_lane_row<S16>(e_lane)) * p.ldr + e_gn;
#define PV_V8_FETCH_RES(MI)                                                                          \
        if constexpr (EPI == PV_EPI_RESID) {                                                         \
            _Pragma("unroll") for (int it = 0; it < 4; ++it)                                         \
                if ((MI) * 32 + epi_pass_row<S16>(it) < e_rows_left)                                 \
                    e_res[MI][it] = *reinterpret_cast<const uint4*>(e_rbase + (int64_t)((MI) * 32 + epi_pass_row<S16>(it)) * p.ldr); \
        }
        // k-step 0's fragments of the tile's first slab (visible since the last barrier of the previous tile's loop; that loop's
        // last refills fetched the same values, but carrying 36 registers across the epilogue costs the loop body spills)
        uint4 fa[MB], fb[2][2];
        g.first_fragments(fa, fb, ringA0, ringB0);
        int kt = 0;
        do {                                                       // (nk2 >= 2 and even: the launcher's condition)
            PV_V8_EVEN(kt)
            if (kt == 0) {
                // The epilogue's operands are fetched HERE -- inside the loop, behind the first slab's wait (which also covered the
                // previous tile's stores) and in front of the second's, which retires them: hipcc then knows them landed when the
                // epilogue reads them.  Fetched in front of the loop, their first use behind it (the next tile's pieces in flight)
                // is answered with a vmcnt(0); named as used inside the loop, the queue is flushed in the loop's preheader.
                PV_V8_EPI_GEOMETRY()
                (void)e_out0;
                if (e_live && e_biasp) e_bias = *reinterpret_cast<const uint4*>(e_biasp + e_col);
                if constexpr (MB < 5) { PV_V8_FETCH_RES(0) }        // (MB = 5: sixteen more registers through the loop body spill)
            }
            PV_V8_ODD(kt + 1)
            kt += 2;
        } while (kt + 2 <= nk2);
        trace_stamp(p.trace, vb, 1);

        // ---- store epilogue: 8 rows x 64 columns per pass through the wave's own 2 KB (the ring holds the next tile)
        PV_V8_EPI_GEOMETRY()
        (void)e_biasp;
        const pv_f32x2 e_b[4] = {unpack2(e_bias.x), unpack2(e_bias.y), unpack2(e_bias.z), unpack2(e_bias.w)};
        const int64_t e_row0 = (int64_t)(m0 + wm * 32 * MB + epi_lane_row<S16>(e_lane)) * p.ldo;
        T* const o0_base = e_out0 ? e_out0 + e_row0 + e_col : nullptr;
        T* const o1_base = reinterpret_cast<T*>(p.out1) + e_row0 + e_gn;
        float* const Cs = reinterpret_cast<float*>(stage + wave * 2048);
        const float* const Cr = Cs + epi_read_off<S16>(e_lane);
        [[maybe_unused]] float* const Cw = Cs + (e_lane >> 5) * 256 + (e_lane & 31);
        if constexpr (MB >= 5) { PV_V8_FETCH_RES(0) }
#pragma unroll
        for (int mi = 0; mi < MB; ++mi) {
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                if constexpr (S16) {
                    stage_pass16(Cs, acc[mi], it, e_lane);
                } else {
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            Cw[j * 64 + ni * 32] = acc[mi][ni][4 * it + j];
                }
                __builtin_amdgcn_wave_barrier();
                if (it == 0) {
                    // residual rows two blocks ahead, as v7
                    if (2 * mi + 1 < MB) { PV_V8_FETCH_RES((2 * mi + 1 < MB ? 2 * mi + 1 : 0)) }
                    if (2 * mi + 2 < MB) { PV_V8_FETCH_RES((2 * mi + 2 < MB ? 2 * mi + 2 : 0)) }
                }
                if (mi * 32 + epi_pass_row<S16>(it) < e_rows_left) {
                    const float4 x0 = *reinterpret_cast<const float4*>(Cr);
                    const float4 x1 = *reinterpret_cast<const float4*>(Cr + 4);
                    const int64_t ro = (int64_t)(mi * 32 + epi_pass_row<S16>(it)) * p.ldo;
                    epi8_bf16<EPI, ACT>(x0, x1, e_b, o0_base ? o0_base + ro : nullptr, o1_base + ro,
                                        e_res[EPI == PV_EPI_RESID ? mi : 0][it]);
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
#undef PV_V8_EPI_GEOMETRY
#undef PV_V8_FETCH_RES
        trace_stamp(p.trace, vb, 2);
        if (!has_next) break;
        kloop::zero(acc);
        vb = vbn; m0 = m0n; n0 = n0n; uA = uAn; uB = uBn;
        trace_stamp(p.trace, vb, 0);
    }
#undef PV_V8_EVEN
#undef PV_V8_ODD
    __builtin_amdgcn_s_waitcnt(0x0F70);     // the dead prefetches behind the last tile must land before the LDS is handed on
}

// the run-time (epi, act) of a launch -> the compile-time pair the kernels are instantiated for: f(EpiAct<EPI, ACT>{})
template <int EPI, int ACT>
struct EpiAct {
    static constexpr int epi = EPI, act = ACT;
};
template <class F>
void with_epi_act(const GemmParams& p, F&& f) {
    if (p.epi == PV_EPI_BIAS) f(EpiAct<PV_EPI_BIAS, 0>{});
    else if (p.epi == PV_EPI_QKV) f(EpiAct<PV_EPI_QKV, 0>{});
    else if (p.epi == PV_EPI_RESID) f(EpiAct<PV_EPI_RESID, 0>{});
    else if (p.act == PV_ACT_GELU) f(EpiAct<PV_EPI_ACT, PV_ACT_GELU>{});
    else if (p.act == PV_ACT_QUICK_GELU) f(EpiAct<PV_EPI_ACT, PV_ACT_QUICK_GELU>{});
    else f(EpiAct<PV_EPI_ACT, PV_ACT_RELU>{});
}

// one launch of a kernel pointer on 512-thread workgroups; timed: the profiler's event pair (prof.hpp) rides on the dispatch packet
struct LaunchTiming {
    bool timed;
    hipEvent_t ev0, ev1;
};
template <typename... P, typename... A>
void launch_kernel(void (*kernel)(P...), int grid, hipStream_t stream, const LaunchTiming& t, const A&... args) {
    if (t.timed) hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(512), 0, stream, t.ev0, t.ev1, 0, args...);
    else hipLaunchKernelGGL(kernel, dim3(grid), dim3(512), 0, stream, args...);
}

template <typename T, int MB>
int launch_tiled(const GemmParams& p, const GemmChoice& c, hipStream_t stream) {
    {
        const GemmCost cost = gemm_cost<T>(p);
        const int stagger = g_pv_tuning.gemm_stagger;
        LaunchTiming t{false, nullptr, nullptr};
        t.timed = !g_pv_tuning.prof_markers && pv_prof_events(PV_PROF_GEMM, cost.flops, cost.bytes, &t.ev0, &t.ev1);
        ProfScope prof(t.timed ? PV_PROF__COUNT : PV_PROF_GEMM, stream, cost.flops, cost.bytes);
        with_epi_act(p, [&](auto ea) {
            constexpr int EPI = decltype(ea)::epi, ACT = decltype(ea)::act;
            if (c.kernel == PV_GEMM_V8) launch_kernel(gemm_kernel_v8<T, MB, EPI, ACT>, c.grid, stream, t, p, c.ntiles, stagger);
            else if (c.LP == 2) launch_kernel(gemm_kernel_v7<T, MB, EPI, ACT, 2>, c.grid, stream, t, p);
            else if (c.LP == 1) launch_kernel(gemm_kernel_v7<T, MB, EPI, ACT, 1>, c.grid, stream, t, p);
            else launch_kernel(gemm_kernel_v7<T, MB, EPI, ACT, 0>, c.grid, stream, t, p);
        });
    }
    PV_LAUNCH_CHECK("gemm_kernel_v7");
    return PV_OK;
}

}  // namespace

int pv_gemm_launch_tiled(const GemmParams& p, const GemmChoice& c, hipStream_t stream) {
    return c.MB == 5 ? launch_tiled<bf16_t, 5>(p, c, stream) : launch_tiled<bf16_t, 4>(p, c, stream);
}
