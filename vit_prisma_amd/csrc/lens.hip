// Patch-level logit lens on the cached residual stream (gfx950).
//
// Reference semantics (prisma_tools/logit_lens.py:20-45): stack the residual stream at the input of every layer plus the final
// one (activation_cache.py:160-292), subtract each row's mean and divide by the CACHED ln_final.hook_scale of the row's token
// (activation_cache.py:656-735: no LayerNorm weight or bias), multiply with the answer directions [O, d] and permute to
// [B, T, S, O].  get_patch_logit_dictionary (logit_lens.py:47-89) then takes, per (token, stack entry), the largest logit, its
// index and the rank of one label.
//
// Here the stack is never built and the normalised rows are never written.  With N = B * T rows per tap, x_s the bf16 tap of
// stack entry s read in place, a^ the answers in bf16, asum[o] = sum_k a^[o, k] and mean_s[n] the row mean (both fp32):
//
//   out[n, s, o] = (sum_k x_s[n, k] a^[o, k]  -  mean_s[n] * asum[o]) / scale[n]
//
// The products are exact on the matrix core and summed in fp32; centring happens on the sum, not on the operand, so no centred
// value is ever rounded to bf16 (the reference rounds the mean and every centred element: 2^-9 relative per element).
//
//   lens_rowstat_kernel     a wave per row: the S * N row means, and in the same launch the O answer sums
//   lens_gemm_kernel        the K loop of gemm_kernel_v7 (kloop.hpp) with a source functor that takes its A rows from ONE of S
//                           tap buffers: row tiles are counted per stack entry (grid = S * ceil(N / TM) x ceil(O / 256)), so a
//                           tile never straddles two taps and the workgroup builds its A descriptor from ptr[s].
//                           MODE 0 stores fp32 at out + ((n * S + s) * O + o) -- the reference's permuted layout.
//                           MODE 1 stores no logits: per (row, N-tile) the maximum, the lowest column holding it, and the count
//                           of columns that rank before the label column (larger, or equal at a lower index)
//   lens_top_finish_kernel  the ceil(O / 256) partials of a row -> top_idx, top_logit, rank
// The label's logit, which MODE 1 compares against, comes from a MODE 0 launch with O = 1 on the label's row of a^: the same K
// loop and epilogue arithmetic, hence the same bits as the label column of the wide launch.
//
// Non-finite rows: a tap row that holds a NaN or an infinity has a non-finite mean in the reference and comes out NaN in every
// column.  The row-stat kernel turns a non-finite mean into NaN, which the epilogue's subtraction spreads over the row (the
// algebraic form alone would leave +-inf where the signs of the two terms differ).  Top-1 of such a row: index 0, NaN; rank -1.
//
// Error of a finite element against the exact value (u = 2^-24, K = d_model): the dot product and the mean are fp32 sums of K
// terms in some order, the epilogue adds one product, one difference and one quotient:
//   |got - exact| <= (K + 4) u (sum_k |x_k a^_k| + |mean| sum_k |a^_k|) / scale         (tests/_lens_cases.py holds it to that)
#include "kloop.hpp"

namespace {

constexpr bool S16 = kloop::Shape<kloop::Bf16>::S16;

struct LensParams {
    const void* ptr[PV_LENS_MAX_STACK];   // the S taps, [N][K] bf16 each
    const void* B;                        // a^ rows [O][K] bf16
    const float* mean;                    // [S][N]
    const float* asum;                    // [O]
    const float* scale;                   // [N]
    int32_t N, S, O, K;
    float* out;                           // MODE 0: [N][S][O]
    const float* lab;                     // MODE 1: [N][S] logit of the label column, or NULL
    int32_t label;                        //         the label column, or -1
    float* pmax;                          //         [N][S][ntn] partials
    int32_t* pidx;
    int32_t* pcnt;
};

// (a_v, a_i) ranks before (b_v, b_i): the larger value, at equal values the lower index -- torch.argmax's order, in which a NaN
// is the largest value there is
__device__ __forceinline__ bool lens_before(float av, int ai, float bv, int bi) {
    const bool an = av != av, bn = bv != bv;
    if (an | bn) return an & (!bn | (ai < bi));
    return (av > bv) | ((av == bv) & (ai < bi));
}

// Where a lane's accumulators sit in its wave's (32 * MB) x 64 tile, for both MFMA shapes (kloop.hpp).  A lane holds NROW rows
// of NCOL columns each; the lanes that share a row differ in the low GROUP bits.
template <int MB>
struct LensEpi {
    static constexpr int NROW = S16 ? 8 * MB : 16 * MB, NCOL = S16 ? 4 : 2, GROUP = S16 ? 16 : 32;
    __device__ static __forceinline__ int row(int lane, int i) {
        if constexpr (S16) return (i >> 2) * 16 + 4 * (lane >> 4) + (i & 3);
        else return (i >> 4) * 32 + (i & 3) + 8 * ((i & 15) >> 2) + 4 * (lane >> 5);
    }
    __device__ static __forceinline__ int col(int lane, int c) {
        if constexpr (S16) return c * 16 + (lane & 15);
        else return c * 32 + (lane & 31);
    }
    __device__ static __forceinline__ float val(const f32x16 (&acc)[MB][2], int i, int c) {
        if constexpr (S16) return acc[i >> 3][c >> 1][4 * (2 * ((i >> 2) & 1) + (c & 1)) + (i & 3)];
        else return acc[i >> 4][c][i & 15];
    }
};

// MB: 32-row blocks per wave along M -- 4 (256 x 256 tiles), or 2 (128 x 256) where a tap has fewer than 256 rows (one image).
// LP: 2 = full-line K slabs (K a whole number of 128-byte slabs: every registry width), 0 = barrier-then-fetch with its K tail.
template <int MODE, int MB, int LP>
__global__ __launch_bounds__(512, 2) void lens_gemm_kernel(const LensParams p) {
    static_assert(MB == 2 || MB == 4, "128- or 256-row tiles");
    static_assert(LP == 0 || LP == 2, "the barrier-then-fetch loop or the full-line loop");
    using R64 = kloop::Ring64<MB, S16>;
    using R128 = kloop::Ring128<MB, false, S16>;
    using E = LensEpi<MB>;
    constexpr int TM = 64 * MB, TN = 256, SLOT = R64::SLOT, NA = R64::NA;
    static_assert(R128::SLOT == 2 * SLOT, "a full-line slot is two 64-byte-slab slots");
    static_assert(!R64::PAD, "every wave has NA real A pieces at MB = 2, 4");
    // the ring slots, one object each (kloop.hpp)
    __shared__ __attribute__((aligned(16))) unsigned char ring0[LP == 2 ? 2 * SLOT : SLOT];
    __shared__ __attribute__((aligned(16))) unsigned char ring1[LP == 2 ? 2 * SLOT : SLOT];
    __shared__ __attribute__((aligned(16))) unsigned char ring2[LP == 2 ? 16 : SLOT];
    __shared__ __attribute__((aligned(16))) unsigned char ring3[LP == 2 ? 16 : SLOT];
    __shared__ __attribute__((aligned(16))) unsigned char pad[16];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    // row tiles are counted per stack entry: tile_m = s * ntm + (row tile inside tap s)
    const int ntm = (p.N + TM - 1) / TM;
    const int swz = kloop::xcd_run(blockIdx.x, gridDim.x);
    const kloop::TileOrder<TM, TN> order(p.S * ntm * TM, p.O);
    int tile_m, tile_n;
    order.at(swz, tile_m, tile_n);
    const int s = tile_m / ntm;
    const int m0 = (tile_m - s * ntm) * TM, n0 = tile_n * TN;

    const unsigned Kb = (unsigned)p.K * 2u;
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<void*>(p.ptr[s]), 0, (int)((unsigned)p.N * Kb), 0x00020000);                      // rows >= N: past the range -> 0
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<void*>(p.B), 0, (int)((unsigned)p.O * Kb), 0x00020000);                           // rows >= O likewise

    f32x16 acc[MB][2];
    kloop::zero(acc);

    if constexpr (LP == 0) {
        const R64 g(lane, wave, pad);
        const int nk = (int)((Kb + 63) / 64);
        const bool ktail = (Kb % 64) != 0;
        unsigned offA[NA], kcA[NA], offB[2], kcB[2];
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            const int row = g.piece_row(lane, j);
            kcA[j] = R64::piece_col(lane, row);
            offA[j] = (unsigned)(m0 + row) * Kb + kcA[j];
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int row = g.piece_row(lane, j);
            kcB[j] = R64::piece_col(lane, row);
            offB[j] = (unsigned)(n0 + row) * Kb + kcB[j];
        }
        auto issue = [&](int kt, unsigned char* slot) {
            const unsigned kbase = (unsigned)kt * 64;
            const bool dead = (kt >= nk);
#pragma unroll
            for (int j = 0; j < NA; ++j)
                g.issue(rsA, rsB, slot, j, (dead | (ktail & (kbase + kcA[j] >= Kb))) ? kloop::DEAD : offA[j] + kbase);
#pragma unroll
            for (int j = 0; j < 2; ++j)
                g.issue(rsA, rsB, slot, NA + j, (dead | (ktail & (kbase + kcB[j] >= Kb))) ? kloop::DEAD : offB[j] + kbase);
        };
        KLOOP_RUN_FETCH_AFTER_BARRIER(kloop::Bf16, acc, g, ring0, ring1, ring2, ring3, nk, issue);
    } else {
        const R128 g(lane, wave);
        const int nk2 = (int)(Kb / 128);
        const unsigned pA0 = (unsigned)(m0 + g.piece_row(lane)) * Kb + g.piece_col(lane);
        const unsigned pB0 = (unsigned)(n0 + g.piece_row(lane)) * Kb + g.piece_col(lane);
        const unsigned stride = R128::PIECE_STRIDE * Kb;
        auto src = [&](int kt, int j) -> unsigned {
            const unsigned kbase = (unsigned)kt * 128;
            const bool dead = (kt >= nk2);
            if (j < MB) return dead ? kloop::DEAD : pA0 + ((unsigned)j * stride + kbase);
            return dead ? kloop::DEAD : pB0 + ((unsigned)(j - MB) * stride + kbase);
        };
        KLOOP_RUN_FULL_LINE(kloop::Bf16, MB, acc, g, rsA, rsB, ring0, ring1, nk2, src);
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);     // vmcnt(0): drain the off-the-end prefetches
    __syncthreads();

    // epilogue: centring on the sum, then the cached scale
    const int wrow0 = m0 + wm * 32 * MB;                  // first row of this wave's block inside tap s
    const int wcol0 = n0 + wn * 64;
    float as[E::NCOL];
#pragma unroll
    for (int c = 0; c < E::NCOL; ++c) {
        const int gc = wcol0 + E::col(lane, c);
        as[c] = gc < p.O ? p.asum[gc] : 0.0f;
    }
    if constexpr (MODE == 0) {
#pragma unroll
        for (int i = 0; i < E::NROW; ++i) {
            const int n = wrow0 + E::row(lane, i);
            if (n < p.N) {
                const float mean = p.mean[(int64_t)s * p.N + n], scale = p.scale[n];
                float* o = p.out + ((int64_t)n * p.S + s) * p.O;
#pragma unroll
                for (int c = 0; c < E::NCOL; ++c) {
                    const int gc = wcol0 + E::col(lane, c);
                    if (gc < p.O) o[gc] = __fdiv_rn(E::val(acc, i, c) - mean * as[c], scale);
                }
            }
        }
    } else {
        // per row of the tile, this wave's 64 columns -> one partial in LDS; then a thread per row folds the four waves' partials
        float* smax = reinterpret_cast<float*>(ring0);                    // [TM][4]
        int* sidx = reinterpret_cast<int*>(ring0 + TM * 16);
        int* scnt = reinterpret_cast<int*>(ring0 + 2 * TM * 16);
        static_assert(3 * TM * 16 <= SLOT, "the partials fit the first ring slot");
#pragma unroll
        for (int i = 0; i < E::NROW; ++i) {
            const int lrow = wm * 32 * MB + E::row(lane, i);
            const int n = m0 + lrow;
            const bool live = n < p.N;
            const float mean = live ? p.mean[(int64_t)s * p.N + n] : 0.0f, scale = live ? p.scale[n] : 1.0f;
            const float lab = (live && p.lab) ? p.lab[(int64_t)n * p.S + s] : 0.0f;
            float bv = -INFINITY;
            int bi = 0x7fffffff, cnt = 0;
#pragma unroll
            for (int c = 0; c < E::NCOL; ++c) {
                const int gc = wcol0 + E::col(lane, c);
                if (gc < p.O) {
                    const float v = __fdiv_rn(E::val(acc, i, c) - mean * as[c], scale);
                    if (lens_before(v, gc, bv, bi)) { bv = v; bi = gc; }
                    const bool before = ((v > lab) | ((v == lab) & (gc < p.label))) & (gc != p.label);
                    cnt += before ? 1 : 0;
                }
            }
#pragma unroll
            for (int o = 1; o < E::GROUP; o <<= 1) {
                const float ov = __shfl_xor(bv, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                cnt += __shfl_xor(cnt, o, 64);
                if (lens_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
            }
            if ((lane & (E::GROUP - 1)) == 0) {
                smax[lrow * 4 + wn] = bv;
                sidx[lrow * 4 + wn] = bi;
                scnt[lrow * 4 + wn] = cnt;
            }
        }
        __syncthreads();
        if (tid < TM && m0 + tid < p.N) {
            float bv = smax[tid * 4];
            int bi = sidx[tid * 4], cnt = scnt[tid * 4];
#pragma unroll
            for (int w = 1; w < 4; ++w) {
                const float ov = smax[tid * 4 + w];
                const int oi = sidx[tid * 4 + w];
                cnt += scnt[tid * 4 + w];
                if (lens_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
            }
            const int64_t at = ((int64_t)(m0 + tid) * p.S + s) * order.ntn + tile_n;
            p.pmax[at] = bv;
            p.pidx[at] = bi;
            p.pcnt[at] = cnt;
        }
    }
}

// the S pointers again, for the row-stat kernel (a struct of its own: it needs nothing else by value)
struct LensTaps {
    const void* ptr[PV_LENS_MAX_STACK];
};

// A wave per row.  Rows [0, S * N): the mean of row n of tap s -> mean[s * N + n], NaN where the sum is not finite.
// Rows [S * N, S * N + O): the sum of answer row o -> asum[o].  K % 8 == 0: 16-byte loads.
__global__ __launch_bounds__(256) void lens_rowstat_kernel(const LensTaps taps, const bf16_t* __restrict__ answers, int N, int S, int O,
                                                           int K, float* __restrict__ mean, float* __restrict__ asum) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t n_tap_rows = (int64_t)S * N;
    if (r >= n_tap_rows + O) return;
    const bool is_tap = r < n_tap_rows;
    const int s = is_tap ? (int)(r / N) : 0;
    const int64_t n = is_tap ? r - (int64_t)s * N : r - n_tap_rows;
    const bf16_t* x = (is_tap ? reinterpret_cast<const bf16_t*>(taps.ptr[s]) : answers) + n * K;
    float sum = 0.0f;
    for (int k = 8 * lane; k < K; k += 512) {
        float v[8];
        load8(x + k, v);
        sum += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    }
    sum = wave_sum(sum);
    if (lane == 0) {
        if (is_tap) {
            const float m = sum / (float)K;
            mean[r] = (fabsf(m) <= 3.402823466e38f) ? m : __uint_as_float(0x7fc00000u);
        } else {
            asum[n] = sum;
        }
    }
}

__global__ __launch_bounds__(256) void lens_top_finish_kernel(const float* __restrict__ pmax, const int32_t* __restrict__ pidx,
                                                              const int32_t* __restrict__ pcnt, const float* __restrict__ lab,
                                                              int64_t rows, int ntn, int32_t* __restrict__ top_idx,
                                                              float* __restrict__ top_logit, int32_t* __restrict__ rank) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    float bv = pmax[r * ntn];
    int bi = pidx[r * ntn], cnt = pcnt[r * ntn];
    for (int t = 1; t < ntn; ++t) {
        const float ov = pmax[r * ntn + t];
        const int oi = pidx[r * ntn + t];
        cnt += pcnt[r * ntn + t];
        if (lens_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (top_idx) top_idx[r] = bi;
    if (top_logit) top_logit[r] = bv;
    if (rank) {
        const float l = lab[r];
        rank[r] = (l != l) ? -1 : cnt;
    }
}

struct LensWorkspace {
    size_t mean, asum, lab, pmax, pidx, pcnt, total;
};
LensWorkspace lens_workspace(int64_t N, int64_t S, int64_t O) {
    const int64_t ntn = (O + 255) / 256;
    LensWorkspace w;
    size_t at = 0;
    auto take = [&](int64_t bytes) { const size_t o = at; at += (size_t)pv_align_up(bytes, 256); return o; };
    w.mean = take(S * N * 4);
    w.asum = take(O * 4);
    w.lab = take(N * S * 4);
    w.pmax = take(N * S * ntn * 4);
    w.pidx = take(N * S * ntn * 4);
    w.pcnt = take(N * S * ntn * 4);
    w.total = at;
    return w;
}

template <int MODE>
int lens_launch_gemm(const LensParams& p, hipStream_t stream) {
    const bool tm256 = p.N >= 256;                       // a tap with fewer rows (one image) runs 128-row tiles
    const int tm = tm256 ? 256 : 128;
    const int ntm = (p.N + tm - 1) / tm, ntn = (p.O + 255) / 256;
    const dim3 grid(p.S * ntm * ntn), block(512);
    const bool full_line = ((int64_t)p.K * 2) % 128 == 0;
    if (tm256) {
        if (full_line) hipLaunchKernelGGL((lens_gemm_kernel<MODE, 4, 2>), grid, block, 0, stream, p);
        else hipLaunchKernelGGL((lens_gemm_kernel<MODE, 4, 0>), grid, block, 0, stream, p);
    } else {
        if (full_line) hipLaunchKernelGGL((lens_gemm_kernel<MODE, 2, 2>), grid, block, 0, stream, p);
        else hipLaunchKernelGGL((lens_gemm_kernel<MODE, 2, 0>), grid, block, 0, stream, p);
    }
    PV_LAUNCH_CHECK("lens_gemm_kernel");
    return PV_OK;
}

}  // namespace

extern "C" size_t pv_logit_lens_workspace_bytes(int32_t n_rows, int32_t n_stack, int32_t d_model, int32_t n_answers) {
    (void)d_model;
    if (n_rows <= 0 || n_stack <= 0 || n_answers <= 0) return 0;
    return lens_workspace(n_rows, n_stack, n_answers).total;
}

extern "C" int pv_logit_lens(int32_t dtype, const void* const* resid, int32_t n_stack, int32_t n_rows, int32_t d_model,
                             const float* scale, const void* answers, int32_t n_answers, float* directions, int32_t* top_idx,
                             float* top_logit, int32_t rank_of, int32_t* rank, void* workspace, size_t workspace_bytes,
                             void* stream_) {
    PV_REQUIRE(dtype == PV_DTYPE_BF16, "logit lens: the taps and the answers must be bf16 (dtype PV_DTYPE_BF16); fp32 is not served");
    PV_REQUIRE(d_model >= 8 && d_model % 8 == 0, "logit lens: d_model must be a multiple of 8 (16-byte operand chunks)");
    PV_REQUIRE(n_stack >= 1 && n_stack <= PV_LENS_MAX_STACK,
               "logit lens: n_stack must be between 1 and PV_LENS_MAX_STACK = " PV_STR(PV_LENS_MAX_STACK));
    PV_REQUIRE(n_rows >= 1 && n_answers >= 1, "logit lens: n_rows and n_answers must be positive");
    const bool want_top = top_idx || top_logit || rank;
    PV_REQUIRE(directions || want_top, "logit lens: no output requested (directions, top_idx, top_logit and rank are all NULL)");
    PV_REQUIRE(!rank || (rank_of >= 0 && rank_of < n_answers), "logit lens: rank needs a label column 0 <= rank_of < n_answers");
    PV_REQUIRE(resid && scale && answers && workspace, "logit lens: resid, scale, answers and workspace must not be NULL");
    PV_REQUIRE(pv_aligned16(answers), "logit lens: answers must be 16-byte aligned");
    for (int s = 0; s < n_stack; ++s)
        PV_REQUIRE(resid[s] && pv_aligned16(resid[s]), "logit lens: every tap must be a 16-byte aligned device pointer");
    const uint64_t kb = (uint64_t)d_model * 2;
    PV_REQUIRE(((uint64_t)n_rows + 256) * kb < 0xffffff00ull && ((uint64_t)n_answers + 256) * kb < 0xffffff00ull,
               "logit lens: a tap and the answers must each stay below 4 GiB (32-bit buffer offsets)");
    const LensWorkspace w = lens_workspace(n_rows, n_stack, n_answers);
    if (workspace_bytes < w.total) {
        pv_set_error("logit lens: workspace too small (pv_logit_lens_workspace_bytes)");
        return PV_ERR_WORKSPACE;
    }
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    unsigned char* ws = reinterpret_cast<unsigned char*>(workspace);

    LensParams p{};
    LensTaps taps{};
    for (int s = 0; s < n_stack; ++s) p.ptr[s] = taps.ptr[s] = resid[s];
    p.mean = reinterpret_cast<float*>(ws + w.mean);
    p.scale = scale;
    p.N = n_rows; p.S = n_stack; p.K = d_model;
    p.label = -1;

    {
        const int64_t rows = (int64_t)n_stack * n_rows + n_answers;
        hipLaunchKernelGGL(lens_rowstat_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, taps,
                           reinterpret_cast<const bf16_t*>(answers), n_rows, n_stack, n_answers, d_model,
                           reinterpret_cast<float*>(ws + w.mean), reinterpret_cast<float*>(ws + w.asum));
        PV_LAUNCH_CHECK("lens_rowstat_kernel");
    }
    if (directions) {
        p.B = answers;
        p.asum = reinterpret_cast<float*>(ws + w.asum);
        p.O = n_answers;
        p.out = directions;
        if (int rc = lens_launch_gemm<0>(p, stream)) return rc;
    }
    if (want_top) {
        float* lab = nullptr;
        if (rank) {
            // the label's logit per (row, stack entry): the directions launch on the label's row alone
            lab = reinterpret_cast<float*>(ws + w.lab);
            p.B = reinterpret_cast<const bf16_t*>(answers) + (int64_t)rank_of * d_model;
            p.asum = reinterpret_cast<float*>(ws + w.asum) + rank_of;
            p.O = 1;
            p.out = lab;
            if (int rc = lens_launch_gemm<0>(p, stream)) return rc;
        }
        p.B = answers;
        p.asum = reinterpret_cast<float*>(ws + w.asum);
        p.O = n_answers;
        p.out = nullptr;
        p.lab = lab;
        p.label = rank ? rank_of : -1;
        p.pmax = reinterpret_cast<float*>(ws + w.pmax);
        p.pidx = reinterpret_cast<int32_t*>(ws + w.pidx);
        p.pcnt = reinterpret_cast<int32_t*>(ws + w.pcnt);
        if (int rc = lens_launch_gemm<1>(p, stream)) return rc;
        const int64_t rows = (int64_t)n_rows * n_stack;
        hipLaunchKernelGGL(lens_top_finish_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, p.pmax, p.pidx, p.pcnt,
                           lab, rows, (n_answers + 255) / 256, top_idx, top_logit, rank);
        PV_LAUNCH_CHECK("lens_top_finish_kernel");
    }
    return PV_OK;
}
