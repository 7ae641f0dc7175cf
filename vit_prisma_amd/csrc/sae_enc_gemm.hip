// The fp16 filter GEMM of the filtered SAE encoder (sae_enc.hip: the top-k form and the error bound of the filter; sae_enc_relu.hip:
// the sparse ReLU / gated form).  Two passes of the top-k form and one of the ReLU form run it:
//   pass 0   on every 16th feature (1/16 of the work) -> sample [N, d_sae/16], plain fp32 (MODE 0)
//   filter   the full encoder product on v_mfma_f32_32x32x16_f16 (operands rounded to fp16); the epilogue keeps no tile -- it appends
//            (j, a_j) for a_j >= T_n to the token's candidate list of the feature's 256-column tile (MODE 1): hits compacted in LDS
//            (at most HCAP per round), one round for the whole tile where the expected hits fit (ONE), else one per 32-row block
// Tiles are walked in gemm_kernel_v7's order, so that a column block's weight panel stays in the XCD's L2.
#include <atomic>

#include "kloop.hpp"
#include "sae_enc.hpp"

namespace {

// The hit epilogue: this lane's first list position for its nh hits -- a wave inclusive scan, then ONE LDS atomic per wave for the base.
// (Not a lambda of the kernel: declared in the kernel template it changed the prologue of the MODE 0 instances, which never use it.)
__device__ __forceinline__ uint32_t enc_wave_pos(uint32_t* hit_n, int nh, int lane) {
    int incl = nh;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    uint32_t base = 0;
    if (lane == 63) base = atomicAdd(hit_n, (uint32_t)incl);
    base = __shfl(base, 63, 64);
    return base + (uint32_t)(incl - nh);
}

// ---------------------------------------------------------------------------------------------------
// filter GEMM: the main loop of gemm_kernel_v7 (kloop.hpp: one 8-wave workgroup per CU, 256 x 256 tile, K slabs DMA'd into an
// LDS ring, counted vmcnt across a raw s_barrier; LP selects the loop form as there) on fp16 operands, with an epilogue that
// stores nothing but the hits.  MODE 0: plain fp32 store of acc + bias (the sample of pass 0).
// ---------------------------------------------------------------------------------------------------
// MB_: 32-row blocks per wave along M -- 4 (256 x 256 tiles) everywhere but the sample pass at the bench shape, whose 4096 x 1536 output
// is 96 such tiles on 256 CUs: 2 (128 x 256 tiles, the full-line loop only) makes it 192 half-sized ones, still one round
template <int MODE, int LP = 0, bool ONE = false, int MB_ = 4>
__global__ __launch_bounds__(512, 2) void sae_enc_gemm_kernel(const EncParams p) {
    constexpr int MB = MB_, TM = 64 * MB, TN = 256;
    static_assert(MB == 4 || (MB == 2 && LP == 2 && MODE == 0), "the 128-row tile exists in the full-line form of the sample pass only");
    using R64 = kloop::Ring64<MB>;
    using R128 = kloop::Ring128<MB>;
    constexpr int SLOT = 64 * (TM + TN);
    // the ring slots, one object each (kloop.hpp).  LP == 2 (full-line K slabs): two slots of 128-byte rows in ring0 / ring1,
    // ring2 / ring3 shrink to stubs
    __shared__ __attribute__((aligned(16))) unsigned char ring0[LP == 2 ? 2 * SLOT : SLOT];
    __shared__ __attribute__((aligned(16))) unsigned char ring1[LP == 2 ? 2 * SLOT : SLOT];
    __shared__ __attribute__((aligned(16))) unsigned char ring2[LP == 2 ? 16 : SLOT];
    __shared__ __attribute__((aligned(16))) unsigned char ring3[LP == 2 ? 16 : SLOT];
    __shared__ __attribute__((aligned(16))) float trow[512];
    __shared__ uint32_t rowcnt[256];
    __shared__ uint32_t hit_n;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    // tile order as in gemm_kernel_v7 (a column block's weight panel -- 8 x 256 rows x K fp16 = 3 MB at K = 768 -- stays in the
    // XCD's L2 while the token rows stream past)
    const int swz = kloop::xcd_run(blockIdx.x, gridDim.x);
    const kloop::TileOrder<TM, TN> order(p.M, p.N);
    const int ntn = order.ntn;
    int tile_m, tile_n;
    order.at(swz, tile_m, tile_n);
    const int m0 = tile_m * TM, n0 = tile_n * TN;

    if constexpr (MODE == 1) {
        if (p.mode) {                                             // (ReLU filter) the step is dense already: nothing to filter
            if (tid == 0) hit_n = __hip_atomic_load(p.mode, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();
            const bool skip = hit_n != 0u;
            __syncthreads();
            if (skip) return;
        }
    }
#ifdef PV_ENC_TRACE
#define ENC_STAMP(slot)                                                                                                    \
    do {                                                                                                                   \
        if (MODE == 1 && p.trace && tid == 0) {                                                                            \
            p.trace[(int64_t)blockIdx.x * 4 + (slot)] = wall_clock64();                                                    \
            if ((slot) == 0) p.trace[(int64_t)blockIdx.x * 4 + 3] = ((uint64_t)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32) | \
                                                                    (uint64_t)__builtin_amdgcn_s_getreg((31 << 11) | 4);    \
        }                                                                                                                  \
    } while (0)
#else
#define ENC_STAMP(slot) do { } while (0)
#endif
    ENC_STAMP(0);
    const unsigned Kb = (unsigned)p.K * 2u;
    const unsigned ldaB = (unsigned)p.lda * 2u;
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<void*>(p.A), 0, (int)((unsigned)p.M * ldaB), 0x00020000);                        // rows >= M land past the range: zero fill
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.B), 0, (int)p.b_span, 0x00020000);

    f32x16 acc[MB][2];
    kloop::zero(acc);
    const int l31 = lane & 31, half = lane >> 5;

    // epilogue operands in flight before the K loop: this lane's two bias values and (MODE 1) the tile's 256 thresholds,
    // DMA'd into LDS (they are the oldest entries of the vmcnt queue, so the first counted wait retires them)
    const int colb = n0 + wn * 64 + l31;
    float bias[2];
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) bias[ni] = (colb + ni * 32 < p.N) ? p.bias[(int64_t)(colb + ni * 32) * p.bias_stride] : 0.0f;
    if constexpr (MODE == 1) {
        const __amdgpu_buffer_rsrc_t rsT = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.thr), 0, p.M * 4, 0x00020000);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsT, (kloop::lds_ptr_t)(trow + wave * 64), 4, (unsigned)(m0 + wave * 64 + lane) * 4u, 0, 0, 0);
    }

    // the K loop (kloop.hpp) on fp16 operands; the B rows (features) past N are made dead explicitly: the descriptor of a strided
    // view of W_enc (the sample pass) does not end where N does
    if constexpr (LP < 2) {
        static_assert(LP == 2 || (R64::NA == 2 && !R64::PAD), "MB = 4: two A pieces and two B pieces per wave per slab");
        const R64 g(lane, wave, nullptr);
        const int nk = (int)((Kb + 63) / 64);
        unsigned offA[2], offB[2], kc[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int row = g.piece_row(lane, j);
            kc[j] = R64::piece_col(lane, row);
            offA[j] = (unsigned)(m0 + row) * ldaB + kc[j];
            offB[j] = (n0 + row < p.N) ? (unsigned)(n0 + row) * p.ldb_bytes + kc[j] : kloop::DEAD;
        }
        if constexpr (LP == 0) {
            const bool ktail = (Kb % 64) != 0;
            auto issue = [&](int kt, unsigned char* slot) {
                const unsigned kbase = (unsigned)kt * 64;
                const bool dead = kt >= nk;
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    g.issue(rsA, rsB, slot, j, (dead | (ktail & (kbase + kc[j] >= Kb))) ? kloop::DEAD : offA[j] + kbase);
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    g.issue(rsA, rsB, slot, 2 + j,
                            (dead | (offB[j] == kloop::DEAD) | (ktail & (kbase + kc[j] >= Kb))) ? kloop::DEAD : offB[j] + kbase);
            };
            KLOOP_RUN_FETCH_AFTER_BARRIER(kloop::F16, acc, g, ring0, ring1, ring2, ring3, nk, issue);
        } else {
            // whole 64-byte slabs only (the launcher checks K % 32 == 0)
            const unsigned strideA = R64::PIECE_STRIDE * ldaB;
            auto src = [&](int kt, int j) -> unsigned {
                const unsigned kbase = (unsigned)kt * 64;
                const bool dead = kt >= nk;
                if (j < 2) return dead ? kloop::DEAD : offA[0] + ((unsigned)j * strideA + kbase);
                const int jb = j >= 2 ? j - 2 : 0;
                return (dead | (offB[jb] == kloop::DEAD)) ? kloop::DEAD : offB[jb] + kbase;
            };
            KLOOP_RUN_PIPELINED64(kloop::F16, MB, acc, g, rsA, rsB, ring0, ring1, ring2, ring3, nk, src);
        }
    } else {
        // whole 128-byte slabs only (the launcher checks K % 64 == 0)
        const R128 g(lane, wave);
        const int nk2 = (int)(Kb / 128);
        const unsigned pA0 = (unsigned)(m0 + g.piece_row(lane)) * ldaB + g.piece_col(lane);
        const int brow0 = n0 + g.piece_row(lane);
        const unsigned pB0 = (unsigned)brow0 * p.ldb_bytes + g.piece_col(lane);
        const unsigned strideA = R128::PIECE_STRIDE * ldaB, strideB = R128::PIECE_STRIDE * p.ldb_bytes;
        auto src = [&](int kt, int j) -> unsigned {
            const unsigned kbase = (unsigned)kt * 128;
            const bool dead = kt >= nk2;
            if (j < MB) return dead ? kloop::DEAD : pA0 + ((unsigned)j * strideA + kbase);
            const int jb = j - MB;
            return (dead | (brow0 + jb * R128::PIECE_STRIDE >= p.N)) ? kloop::DEAD : pB0 + ((unsigned)jb * strideB + kbase);
        };
        KLOOP_RUN_FULL_LINE(kloop::F16, MB, acc, g, rsA, rsB, ring0, ring1, nk2, src);
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);     // vmcnt(0): drain the off-the-end prefetches (and the threshold DMA)
    __syncthreads();
    ENC_STAMP(2);

    const int rows_left = p.M - (m0 + wm * 32 * MB);       // local row r of this wave's block is real iff r < rows_left
    if constexpr (MODE == 0) {
#pragma unroll
        for (int mi = 0; mi < MB; ++mi)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * half;
                if (row < rows_left) {
                    float* o = p.out + (int64_t)(m0 + wm * 32 * MB + row) * p.ldo + colb;
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni)
                        if (colb + ni * 32 < p.N) o[ni * 32] = acc[mi][ni][e] + bias[ni];
                }
            }
    } else {
        // Hits are ~0.8 % of the tile (~2 per token row).  Nothing global is contended for them: every (token, N-tile) pair
        // owns pv_sae_tile_slots() candidate slots and a count word that only this workgroup writes (a device-scope atomic
        // per hit on per-token counters cost more than the whole K loop: ~0.8 M atomics per step queue up behind a few dozen
        // memory channels).  The hits are compacted into LDS with no round trip -- a lane builds the bitmaps of its
        // accumulators, a wave scan + ONE LDS atomic per wave hands out list positions -- then every
        // list entry draws its slot from an LDS per-row counter and is stored.  Rows with more hits than slots (or a tile
        // with more than HCAP hits: massive ties) are marked overflowed: those tokens take the exact path.
        constexpr int HCAP = (LP == 2 ? 2 * SLOT : SLOT) / 8;     // (ring0: SLOT bytes, 2 SLOT in the full-line form)
        uint2* hlist = reinterpret_cast<uint2*>(ring0);
        if (tid == 0) hit_n = p.mode ? __hip_atomic_load(p.mode, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        __syncthreads();                                           // (ONE read of the word per workgroup)
        const bool dense_already = hit_n != 0u;
        __syncthreads();
        if (dense_already) {
            // the step is dense already -- half of all features positive, as at the start of a run: compacting ~32 K hits per tile
            // would cost more than the K loop
            if (tid < 256 && m0 + tid < p.M) p.cnt[(int64_t)(m0 + tid) * ntn + tile_n] = 0xffffffffu;
            return;
        }
        if (tid == 0) hit_n = 0u;
        if (tid < 256) rowcnt[tid] = 0u;
        __syncthreads();
        const float* trw = trow + wm * 32 * MB;
        // bitmap of the hits among this lane's 32 accumulators of block mi: bit (g * 8 + s * 2 + ni)
        auto block_mask = [&](int mi) {
            uint32_t m = 0;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int r0 = mi * 32 + 8 * g + 4 * half;
                const float4 t4 = *reinterpret_cast<const float4*>(trw + r0);
                const float tt[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni) {
                        const bool hit = (r0 + s < rows_left) && (acc[mi][ni][4 * g + s] + bias[ni] >= tt[s]);
                        m |= (hit ? 1u : 0u) << (g * 8 + s * 2 + ni);
                    }
            }
            return m;
        };
        // the hits of block mi into the list from position pos on (returns the next position)
        // (eb: the bias values again, behind an asm barrier in the one-round form -- otherwise hipcc keeps all 128 sums acc + bias
        // of the bitmap pass alive for this one and spills)
        float eb[2] = {bias[0], bias[1]};
        auto block_emit = [&](int mi, uint32_t m, uint32_t pos) {
            if (m != 0u) {
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int s = 0; s < 4; ++s)
#pragma unroll
                        for (int ni = 0; ni < 2; ++ni) {
                            if (m & (1u << (g * 8 + s * 2 + ni))) {
                                const int lrow = wm * 32 * MB + mi * 32 + 8 * g + 4 * half + s;
                                if (pos < (uint32_t)HCAP)
                                    hlist[pos] = make_uint2((uint32_t)(lrow << 8 | (wn * 64 + ni * 32 + l31)),
                                                            __float_as_uint(acc[mi][ni][4 * g + s] + eb[ni]));
                                else
                                    atomicOr(&rowcnt[lrow], 0x80000000u);
                                ++pos;
                            }
                        }
            }
            return pos;
        };
        // list entries [0, nhit) -> each draws its slot from the LDS per-row counter and is stored
        auto flush = [&](uint32_t nhit) {
            for (uint32_t e = tid; e < nhit; e += 512) {
                const uint2 h = hlist[e];
                const int lrow = (int)(h.x >> 8);
                const uint32_t li = atomicAdd(&rowcnt[lrow], 1u) & 0x7fffffffu;
                if (li < (uint32_t)p.slots)
                    p.cand[((int64_t)(m0 + lrow) * ntn + tile_n) * p.slots + li] = make_int2(n0 + (int)(h.x & 255u), (int)h.y);
            }
        };
        // ONE (the launcher: expected hits per tile = 256 rows x slots / 4 -- the slot count is 4 x the mean + 6 -- fit the list
        // twice over: the bench shape, the ReLU filter): one compaction round for the whole tile -- all bitmaps, one wave scan, one
        // LDS atomic per wave, one flush.  Otherwise (small d_sae, large k) a round per 32-row block, each with its own flush.
        if constexpr (ONE) {
            uint32_t mk[MB];
            int nh = 0;
#pragma unroll
            for (int mi = 0; mi < MB; ++mi) {
                mk[mi] = block_mask(mi);
                nh += __popc(mk[mi]);
            }
            asm volatile("" : "+v"(eb[0]), "+v"(eb[1]));
            if (__ballot(nh != 0) != 0ull) {                       // (wave-uniform)
                uint32_t pos = enc_wave_pos(&hit_n, nh, lane);
#pragma unroll
                for (int mi = 0; mi < MB; ++mi) pos = block_emit(mi, mk[mi], pos);
            }
            __syncthreads();
            flush(min(hit_n, (uint32_t)HCAP));
            __syncthreads();
        } else {
            uint32_t flushed = 0;                                  // list positions below this were flushed by earlier blocks
#pragma unroll
            for (int mi = 0; mi < MB; ++mi) {                      // one 32-row block (64 rows of the tile) per round
                const uint32_t m = block_mask(mi);
                if (__ballot(m != 0u) != 0ull)                     // (wave-uniform)
                    block_emit(mi, m, enc_wave_pos(&hit_n, __popc(m), lane) - flushed);
                // flush this block's hits (beyond HCAP of the block's 64 x 256 elements the rows are marked overflowed above).
                // hit_n keeps counting; `flushed` rebases the positions of the next block.
                __syncthreads();
                const uint32_t total = hit_n;
                flush(min(total - flushed, (uint32_t)HCAP));
                flushed = total;
                __syncthreads();
            }
        }
        ENC_STAMP(1);
        if (tid < 256 && m0 + tid < p.M) {
            const uint32_t c = rowcnt[tid];
            p.cnt[(int64_t)(m0 + tid) * ntn + tile_n] = c > (uint32_t)p.slots ? 0xffffffffu : c;
            const bool over = p.mode && c > (uint32_t)p.slots;
            const unsigned long long who = __ballot(over);         // one atomic per wave, not one per overflowed row: on a dense batch
            if (who != 0ull && lane == __ffsll((long long)who) - 1) atomicOr(p.mode, 1u);      // every row of the first 256 tiles overflows
        }
    }
}

// CUs of the current device (cached per device id)
int enc_cus() {
    static std::atomic<int> per_dev[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    int n = per_dev[dev].load(std::memory_order_relaxed);
    if (n == 0) {
        hipDeviceProp_t prop;
        n = hipGetDeviceProperties(&prop, dev) == hipSuccess ? prop.multiProcessorCount : 256;
        if (n <= 0) n = 256;
        per_dev[dev].store(n, std::memory_order_relaxed);
    }
    return n;
}

template <int MODE, int LP, bool ONE = false, int MB = 4>
void enc_launch(dim3 grid, const EncParams& p, hipStream_t stream) {
    hipLaunchKernelGGL((sae_enc_gemm_kernel<MODE, LP, ONE, MB>), grid, dim3(512), 0, stream, p);
}
}  // namespace

int launch_enc_gemm(int mode, const EncParams& p, hipStream_t stream) {
    const int ntm = (p.M + 255) / 256, ntn = (p.N + 255) / 256;
    const dim3 grid(ntm * ntn);
    // K loop as in gemm.hip's launcher: 2 = full-line form (whole 128-byte slabs of fp16: K % 64 == 0), 1 = pipelined 64-byte
    // slabs (K % 32 == 0), 0 = barrier-then-fetch
    int lp = 0;
    if (g_pv_tuning.gemm_loop != 0 && p.K % 32 == 0) lp = (p.K % 64 == 0 && g_pv_tuning.gemm_loop != 1) ? 2 : 1;
    if (mode == 0 && g_pv_tuning.gemm_loop == -1 && p.K % 64 == 0 && ntm * ntn <= enc_cus() / 2 && !g_pv_tuning.enc_tm256)
        // the sample pass where 256-row tiles leave most of the chip idle: 128-row tiles (see the kernel's MB_)
        enc_launch<0, 2, false, 2>(dim3(((p.M + 127) / 128) * ntn), p, stream);
    else if (mode == 0 && lp == 2) enc_launch<0, 2>(grid, p, stream);
    else if (mode == 0 && lp == 1) enc_launch<0, 1>(grid, p, stream);
    else if (mode == 0) enc_launch<0, 0>(grid, p, stream);
    else if (lp == 2 && p.slots * 128 <= 2 * 256 * 128 / 8 && !g_pv_tuning.enc_rounds) enc_launch<1, 2, true>(grid, p, stream);      // (ONE: see the kernel)
    else if (lp == 2) enc_launch<1, 2>(grid, p, stream);
    else if (lp == 1) enc_launch<1, 1>(grid, p, stream);
    else enc_launch<1, 0>(grid, p, stream);
    PV_LAUNCH_CHECK("sae_enc_gemm_kernel");
    return PV_OK;
}
