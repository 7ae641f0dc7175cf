// gemm_kernel_v4 and its launcher: 128 x 128 tile, operands DMA'd straight into a three-slot LDS ring, three workgroups per CU; fp32
// and bf16, plain 16-byte-legal operands (index of the GEMM files: gemm.hip).
// A file of its own, but NOT a translation unit of its own: gemm.hip includes it, once, beside gemm_tiled.hpp.  hipcc propagates the argument ranges
// of all call sites in a translation unit into a device helper before it inlines it, and the persistent kernel calls stage_pass16
// with a lane id of unknown range: compiled without that call in sight, gemm_kernel_v4<bf16> comes out one VGPR and two
// instructions different (MEASURED.md).  Giving it a file to compile alone is a change of its code, to be made with an A/B run.
#pragma once
#include "gemm_epi.hpp"

namespace {

// ---------------------------------------------------------------------------------------------------
// v4 mainloop: operands DMA'd straight into LDS (buffer_load ... lds), deep enough to cover the latency
// (history of the variants in between -- register staging, 2-stage DMA, 128-byte slabs -- in profiles/r01_notes.md).
//   * K slabs of 64 BYTES per row (32 bf16 / 16 fp32): a stage is 8 KB (A) + 8 KB (B)
//   * THREE-stage LDS ring (48 KB) -> 3 workgroups per CU (12 waves): while one workgroup sits at its
//     barrier or in its store epilogue the other two keep the matrix pipe busy
//   * slab k+2 is issued while slab k is multiplied; the wait before the barrier is a COUNTED
//     s_waitcnt vmcnt(4) (only slab k has to have landed, the 4 DMA instructions of slab k+1 stay in
//     flight across the raw s_barrier) -- __syncthreads() would drain the queue
//   * 64-byte rows: 4 chunks per row, 4 rows per 256-byte bank row; chunk position = k-chunk ^ ((row>>2)&3)
//     applied on the DMA source address and on the fragment reads (conflict-free ds_read_b128)
//   * epilogue staged through LDS in two 32-row halves per wave (34.8 KB <= the ring) 
// ---------------------------------------------------------------------------------------------------
using kloop::lds_ptr_t;
constexpr int V4_SLAB = 64;                 // bytes of K per row per stage
constexpr int V4_TILE = 128 * V4_SLAB;      // 8 KB per operand
constexpr int V4_STAGE = 2 * V4_TILE;
constexpr int V4_NSTAGE = 3;
static_assert(V4_NSTAGE * V4_STAGE == 49152, "three 16 KB ring slots -> 3 workgroups per CU");

template <typename T>
__global__ __launch_bounds__(256, 3) void gemm_kernel_v4(const GemmParams p) {
    // One static __shared__ object per ring slot: hipcc's waitcnt pass can then prove that the ds_reads of
    // slot i do not alias the DMA writes in flight to slots i+1 / i+2 (alias scopes per LDS variable); with a
    // single array it inserts s_waitcnt vmcnt(0) before the first ds_read of every step and drains the ring.
    __shared__ __attribute__((aligned(16))) unsigned char ring0[V4_STAGE];
    __shared__ __attribute__((aligned(16))) unsigned char ring1[V4_STAGE];
    __shared__ __attribute__((aligned(16))) unsigned char ring2[V4_STAGE];
    constexpr int EB = DT<T>::kBytes;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int bid = blockIdx.x;
    const int swz = kloop::xcd_run(bid, gridDim.x);
    int tile_m, tile_n;
    kloop::TileOrder<BM, BN>(p.M, p.N).at(swz, tile_m, tile_n);
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    trace_stamp(p.trace, bid, 0);

    const unsigned Kb = (unsigned)p.K * EB;
    const int nk = (int)((Kb + V4_SLAB - 1) / V4_SLAB);
    const bool ktail = (Kb % V4_SLAB) != 0;
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<void*>(p.A), 0, (int)((unsigned)p.M * (unsigned)p.lda * EB), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<void*>(p.Bt), 0, (int)((unsigned)p.N * (unsigned)p.ldb * EB), 0x00020000);

    // 8 wave-instructions (1 KiB = 16 rows x 64 B) per operand per slab; wave w issues instructions 2w, 2w+1
    unsigned offA[2], offB[2], kcb[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int row = (wave * 2 + j) * 16 + (lane >> 2);
        const int kc = (lane & 3) ^ kloop::swz64(row);
        kcb[j] = kc * 16;
        offA[j] = (unsigned)(m0 + row) * (unsigned)p.lda * EB + kc * 16;
        offB[j] = (unsigned)(n0 + row) * (unsigned)p.ldb * EB + kc * 16;
    }
    auto issue = [&](int kt, unsigned char* slot) {
        const unsigned kbase = (unsigned)kt * V4_SLAB;
        unsigned char* Ab = slot + wave * 2048;
        unsigned char* Bb = Ab + V4_TILE;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            unsigned oa = offA[j] + kbase, ob = offB[j] + kbase;
            // NOTE: no branch may surround these DMA instructions -- hipcc's waitcnt pass answers a
            // conditionally executed LDS-DMA with s_waitcnt vmcnt(0) before the next ds_read (ring drained)
            // (bitwise, not short-circuit: it has to compile to selects)
            bool oob = (kt >= nk) | (ktail & (kbase + kcb[j] >= Kb));
#ifdef PV_TUNING
            oob |= (((p.dbg & 1) != 0) & (kt >= 2));
#endif
            oa = oob ? 0xffffff00u : oa;
            ob = oob ? 0xffffff00u : ob;
#ifdef PV_TUNING
            oa = (p.dbg & 4) ? lane * 16u : oa;                     // ablation: every DMA hits the same cached 1 KiB
            ob = (p.dbg & 4) ? lane * 16u : ob;
#endif
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_ptr_t)(Ab + j * 1024), 16, oa, 0, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_ptr_t)(Bb + j * 1024), 16, ob, 0, 0, 0);
        }
    };

    // bf16 on 16x16x32: 4 x 4 accumulators of f32x4, a slab is one k-step (kloop.hpp); fp32 and -DPV_GEMM_MFMA=32: 2 x 2 of f32x16
    constexpr bool W16 = EB == 2 && S16;
    f32x16 acc[2][2];
    kloop::zero(acc);

    const int l31 = lane & 31, half = lane >> 5;
    const int frow = W16 ? (lane & 15) : l31;
    const int sw = kloop::swz64(frow);
    const int co0 = W16 ? ((lane >> 4) ^ sw) * 16 : ((0 + half) ^ sw) * 16, co1 = ((2 + half) ^ sw) * 16;
    const int a_row = (wm * 64 + frow) * V4_SLAB;
    const int b_row = (wn * 64 + frow) * V4_SLAB;
    auto compute = [&](const unsigned char* slot) {
        const unsigned char* Ab = slot;
        const unsigned char* Bb = slot + V4_TILE;
        if constexpr (W16) {
            uint4 a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                a[i] = *reinterpret_cast<const uint4*>(Ab + a_row + i * 16 * V4_SLAB + co0);
                b[i] = *reinterpret_cast<const uint4*>(Bb + b_row + i * 16 * V4_SLAB + co0);
            }
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni)
                    kloop::mfma16_at(kloop::Bf16{}, acc[mi >> 1][ni >> 1], 2 * (mi & 1) + (ni & 1), a[mi], b[ni]);
        } else {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int co = j == 0 ? co0 : co1;
            uint4 a[2], b[2];
            a[0] = *reinterpret_cast<const uint4*>(Ab + a_row + co);
            a[1] = *reinterpret_cast<const uint4*>(Ab + a_row + 32 * V4_SLAB + co);
            b[0] = *reinterpret_cast<const uint4*>(Bb + b_row + co);
            b[1] = *reinterpret_cast<const uint4*>(Bb + b_row + 32 * V4_SLAB + co);
            if constexpr (EB == 2) {
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni)
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                            __builtin_bit_cast(bf16x8, a[mi]), __builtin_bit_cast(bf16x8, b[ni]), acc[mi][ni], 0, 0, 0);
            } else {
                const uint32_t au[2][4] = {{a[0].x, a[0].y, a[0].z, a[0].w}, {a[1].x, a[1].y, a[1].z, a[1].w}};
                const uint32_t bu[2][4] = {{b[0].x, b[0].y, b[0].z, b[0].w}, {b[1].x, b[1].y, b[1].z, b[1].w}};
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                        for (int ni = 0; ni < 2; ++ni)
                            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(
                                __uint_as_float(au[mi][e]), __uint_as_float(bu[ni][e]), acc[mi][ni], 0, 0, 0);
            }
        }
        }
    };
    // one pipeline step: slab kt lives in `cur`, slab kt+2 is issued into `nxt2` (the slot multiplied in step kt-1)
    //   s_waitcnt vmcnt(4): this wave's 4 DMA instructions of slab kt have landed, the 4 of slab kt+1 may
    //   still be in flight (simm16 0x0F74 = vmcnt 4, expcnt 7, lgkmcnt 15: only vmcnt is waited on)
#define PV_V4_STEP(KT, CUR, NXT2)                      \
    __builtin_amdgcn_s_waitcnt(0x0F74);                \
    __builtin_amdgcn_s_barrier();                      \
    issue((KT) + 2, NXT2);                             \
    compute(CUR);

    // Epilogue operands fetched BEFORE the K loop (bf16 only: 40 VGPRs): this lane's 8 bias values and, for the
    // residual epilogues, its 8 x 16 B of residual-stream rows.  They are older than every DMA in the vmcnt
    // queue, so the counted waits of the loop retire them for free and the store epilogue never waits on HBM.
    const int e_gn = n0 + wn * 64 + (lane & 7) * 8;
    const bool e_fast = EB == 2 && p.vec_out && e_gn + 8 <= p.N;
    uint4 e_bias = make_uint4(0, 0, 0, 0);        // 8 raw bf16 (converted in the epilogue: no wait up here)
    uint4 e_res[2][4];
    int e_col = e_gn;
    T* e_out0 = reinterpret_cast<T*>(p.out0);
    if constexpr (EB == 2) {
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int it = 0; it < 4; ++it) e_res[mi][it] = make_uint4(0, 0, 0, 0);
        if (e_fast) {
            const T* bias = reinterpret_cast<const T*>(p.bias0);
            if (p.epi == PV_EPI_QKV) {
                const int which = e_gn / p.nsplit;
                e_col = e_gn - which * p.nsplit;
                if (which == 1) { e_out0 = reinterpret_cast<T*>(p.out1); bias = reinterpret_cast<const T*>(p.bias1); }
                if (which == 2) { e_out0 = reinterpret_cast<T*>(p.out2); bias = reinterpret_cast<const T*>(p.bias2); }
            }
            if (bias) e_bias = *reinterpret_cast<const uint4*>(bias + e_col);
            if (p.epi == PV_EPI_RESID) {
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int it = 0; it < 4; ++it) {
                        const int gm = m0 + wm * 64 + mi * 32 + epi_pass_row<W16>(it) + epi_lane_row<W16>(lane);
                        if (gm < p.M)
                            e_res[mi][it] = *reinterpret_cast<const uint4*>(
                                reinterpret_cast<const T*>(p.resid) + (int64_t)gm * p.ldr + e_gn);
                    }
            }
        }
    }

    issue(0, ring0);
    issue(1, ring1);
    int kt = 0;
    for (; kt + 3 <= nk; kt += 3) {
        PV_V4_STEP(kt, ring0, ring2)
        PV_V4_STEP(kt + 1, ring1, ring0)
        PV_V4_STEP(kt + 2, ring2, ring1)
    }
    if (kt < nk) { PV_V4_STEP(kt, ring0, ring2) }
    if (kt + 1 < nk) { PV_V4_STEP(kt + 1, ring1, ring0) }
#undef PV_V4_STEP
    __builtin_amdgcn_s_waitcnt(0x0F70);     // vmcnt(0): drain the off-the-end prefetches
    __syncthreads();
    trace_stamp(p.trace, bid, 1);
#ifdef PV_TUNING
    if (p.dbg & 2) {
        if (acc[0][0][0] == 123.456f) reinterpret_cast<float*>(p.out0)[0] = acc[1][1][3] + acc[0][1][2] + acc[1][0][1];
        return;
    }
#endif

    // ---- epilogue in two 32-row halves per wave; staging 32 x 64 floats per wave (waves 0,1 in ring0,
    //      waves 2,3 in ring1)
    constexpr int CLD = 64;
    float* Cs = reinterpret_cast<float*>((wave < 2 ? ring0 : ring1) + (wave & 1) * (32 * CLD * 4));
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
        if constexpr (W16) {
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
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int cc = (lane & 7) * 8;
            const int gm = m0 + wm * 64 + mi * 32 + epi_pass_row<W16>(it) + epi_lane_row<W16>(lane);
            const int gn = n0 + wn * 64 + cc;
            if (gm < p.M && gn < p.N) {
                float v[8];
                const float* Cr = Cs + it * 8 * CLD + epi_read_off<W16>(lane);
                const float4 x0 = *reinterpret_cast<const float4*>(Cr);
                const float4 x1 = *reinterpret_cast<const float4*>(Cr + 4);
                v[0] = x0.x; v[1] = x0.y; v[2] = x0.z; v[3] = x0.w;
                v[4] = x1.x; v[5] = x1.y; v[6] = x1.z; v[7] = x1.w;
                if constexpr (EB == 2) {
                    if (e_fast) epilogue8_pre<T>(p, v, gm, gn, e_col, e_out0, e_bias, e_res[mi][it]);
                    else epilogue8<T>(p, v, gm, gn);
                } else {
                    epilogue8<T>(p, v, gm, gn);
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    trace_stamp(p.trace, bid, 2);
}

template <typename T>
int launch_v4(const GemmParams& p, const GemmChoice& c, hipStream_t stream) {
    {
        const GemmCost cost = gemm_cost<T>(p);
        ProfScope prof(PV_PROF_GEMM, stream, cost.flops, cost.bytes);
        hipLaunchKernelGGL((gemm_kernel_v4<T>), dim3(c.grid), dim3(256), 0, stream, p);
    }
    PV_LAUNCH_CHECK("gemm_kernel_v4");
    return PV_OK;
}

}  // namespace

int pv_gemm_launch_v4(int dtype, const GemmParams& p, const GemmChoice& c, hipStream_t stream) {
    return dtype == PV_DTYPE_BF16 ? launch_v4<bf16_t>(p, c, stream) : launch_v4<float>(p, c, stream);
}
