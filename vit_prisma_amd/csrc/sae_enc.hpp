// The filtered SAE encoder's shared pieces: the filter GEMM's parameters (sae_enc_gemm.hip) and the device code that the top-k form
// (sae_enc.hip, whose header derives the error band B_n) and the sparse ReLU / gated form (sae_enc_relu.hip) both run -- one copy of
// each, because the planted suite (tests/_sae_encoder_cases.py) pins this arithmetic bit for bit in both.
#pragma once
#include "sae.hpp"

struct EncParams {
    const void* A;            // [M][lda] fp16
    const void* B;            // fp16 rows; row of output column c starts at B + c * ldb_bytes
    const float* bias;        // bias of column c = bias[c * bias_stride]
    int32_t M, N, K, lda;
    uint32_t ldb_bytes, b_span;
    int32_t bias_stride;
    float* out;               // MODE 0: [M][ldo] fp32 (sample)
    int32_t ldo;
    const float* thr;         // MODE 1: [M] thresholds
    uint32_t* cnt;            //         [M][ntn] hits of (token, N-tile); 0xffffffff = more than `slots`
    int2* cand;               //         [M][ntn][slots] (feature, bits of a)
    int32_t slots;            //         pv_sae_tile_slots(plan)
    uint64_t* trace;          // debug build (-DPV_ENC_TRACE): per-workgroup wall-clock stamps {start, K loop done, end, hw id}, else unused
    uint32_t* mode;           // ReLU filter (pv_sae_relu_step) or NULL: the step's mode word -- a row with more hits than slots raises it
                              // (the step then runs dense), and a tile that finds it raised skips its hit lists
};
// sae_enc_gemm.hip: mode 0 = the sample pass (plain fp32 store), 1 = the filter pass (hit lists)
int launch_enc_gemm(int mode, const EncParams& p, hipStream_t stream);
// sae_enc.hip: *wmax = max_j enc_colsq[j], feat_cnt (or NULL) and *fb_count zeroed (enc_wmax_body in a launch of its own)
int launch_enc_wmax(const float* enc_colsq, int d_sae, float* wmax, uint32_t* fb_count, uint32_t* feat_cnt, hipStream_t stream);
// sae_enc_relu.hip: workgroups of relu_select_kernel<3, false> the runtime says fit a CU (pv_debug_select_occupancy, sae_enc.hip)
int relu_select_occupancy(int* n);

// The error band of the fp16 filter (sae_enc.hip's header) without its rounding term: B_n = ||x_n|| (C1 Wmax + C2) + C2 Wmax
__device__ __forceinline__ float enc_c1(int K) { return fmaxf(1.25e-3f, 9.7680092e-4f + 5.0f * 5.9604645e-8f * (float)K); }
__device__ __forceinline__ float enc_band(float xnorm_n, float wmax_sq, int d_in) {
    const float wmx = sqrtf(wmax_sq);
    const float c2 = 2.98023224e-8f * sqrtf((float)d_in);
    return xnorm_n * (enc_c1(d_in) * wmx + c2) + c2 * wmx;
}

// The weight bound max_j colsq[j] of the band (a NaN column norm poisons it: -> exact fallback) + the zeroing of the per-feature pair
// counters the select kernels draw list positions from, and of the fallback count.  One 256-thread workgroup for d_sae values, the
// long pole of whichever launch carries it: 16-byte accesses, all of a thread's loads in flight at once.  Needs d_sae % 4 == 0 (a plan
// requirement) and 16-byte aligned colsq and feat_cnt (a state tensor; a 256-byte aligned piece of a workspace).
__device__ __forceinline__ void enc_wmax_body(const float* __restrict__ colsq, int d_sae, float* __restrict__ wmax_out,
                                              uint32_t* __restrict__ fb_count, uint32_t* __restrict__ feat_cnt) {
    __shared__ float red[4];
    const int n4 = d_sae >> 2;
    if (feat_cnt)
        for (int j = threadIdx.x; j < n4; j += 256) reinterpret_cast<uint4*>(feat_cnt)[j] = make_uint4(0u, 0u, 0u, 0u);
    float m = 0.f;
    constexpr int WM_FL = 12;                                  // (the bench shape: two round trips to memory; 24 in flight cost the launch its occupancy)
    for (int j0 = threadIdx.x; j0 < n4; j0 += WM_FL * 256) {
        float4 c[WM_FL];
#pragma unroll
        for (int u = 0; u < WM_FL; ++u) c[u] = j0 + u * 256 < n4 ? reinterpret_cast<const float4*>(colsq)[j0 + u * 256] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int u = 0; u < WM_FL; ++u) {
            const float e[4] = {c[u].x, c[u].y, c[u].z, c[u].w};
#pragma unroll
            for (int i = 0; i < 4; ++i) m = (e[i] == e[i]) ? fmaxf(m, e[i]) : INFINITY;      // a NaN column norm poisons the bound (-> exact fallback)
        }
    }
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        *wmax_out = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        *fb_count = 0u;
    }
}

// A token's candidates, as the filter GEMM left them: ntn (<= 256: d_sae <= 65536) per-tile lists of <= slots entries.  Thread t < ntn
// owns tile t: myc = its count, off = where its entries start in the token's list, n = the token's total; bad = the list cannot be
// used: a tile overflowed (sh_bad, which the caller has set -- to 0, or to 1 for "nothing to gather" -- ahead of this call's first
// barrier, is raised) or more than `most` entries.  (Tested by the caller, relu_select_kernel<1, true> takes 66 VGPRs instead of 50
// and loses its eighth wave; tested here, sae_select_kernel<5, true> spills 12 bytes per lane instead of 8.  So the ReLU form passes
// PV_SAE_CAND_CAP, and the top-k form ~0u and tests its two bounds itself.)
// skip: read no counts at all.  256 threads, two barriers; tcnt[256] is free again once every thread is past the call.
struct EncSpan { uint32_t myc, off, n; bool bad; };
__device__ __forceinline__ EncSpan enc_cand_span(const uint32_t* __restrict__ tile_cnt, int64_t row, int ntn, uint32_t* tcnt, uint32_t* sh_bad,
                                                 bool skip, uint32_t most) {
    const int tid = threadIdx.x;
    EncSpan s = {0u, 0u, 0u, false};
    if (tid < ntn && !skip) s.myc = tile_cnt[row * ntn + tid];
    tcnt[tid] = tid < ntn ? s.myc : 0u;
    __syncthreads();
    if (tid < ntn && s.myc == 0xffffffffu) *sh_bad = 1u;
    __syncthreads();
    s.bad = *sh_bad != 0u;
    if (!s.bad) {
        for (int t = 0; t < ntn; ++t) {
            const uint32_t c = tcnt[t];
            s.off += t < tid ? c : 0u;
            s.n += c;
        }
        s.bad = s.n > most;
    }
    return s;
}

// Exact fp32 re-scoring of the nr features in list[] against the token's row x_row: a wave per candidate, four candidates (4 x V4
// 16-byte loads per lane) in flight; emit(c, feature, x . W_encT[feature]) runs on lanes 0..3 for every list position c < nr.
template <int V4, class Emit>
__device__ __forceinline__ void enc_rescore(const float* __restrict__ W_encT, const float* __restrict__ x_row, int d, const int32_t* list,
                                            uint32_t nr, int wave, int lane, Emit emit) {
    bool ok[V4];
    int col[V4];
    float4 xr[V4];
#pragma unroll
    for (int i = 0; i < V4; ++i) {
        col[i] = 4 * lane + 256 * i;
        ok[i] = col[i] < d;
        xr[i] = ok[i] ? *reinterpret_cast<const float4*>(x_row + col[i]) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (uint32_t c0 = wave; c0 < nr; c0 += 16) {
        int jj[4];
        float acc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t c = c0 + 4 * u;
            jj[u] = list[c < nr ? c : c0];
            const float* w = W_encT + (int64_t)jj[u] * d;
            float a = 0.f;
#pragma unroll
            for (int i = 0; i < V4; ++i) {
                if (ok[i]) {
                    const float4 wv = *reinterpret_cast<const float4*>(w + col[i]);
                    a = fmaf(xr[i].x, wv.x, a); a = fmaf(xr[i].y, wv.y, a); a = fmaf(xr[i].z, wv.z, a); a = fmaf(xr[i].w, wv.w, a);
                }
            }
            acc[u] = a;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] += __shfl_xor(acc[u], o, 64);
        if (lane < 4) {
            const uint32_t c = c0 + 4 * lane;
            const float av = lane == 0 ? acc[0] : (lane == 1 ? acc[1] : (lane == 2 ? acc[2] : acc[3]));
            const int jv = lane == 0 ? jj[0] : (lane == 1 ? jj[1] : (lane == 2 ? jj[2] : jj[3]));
            if (c < nr) emit(c, jv, av);
        }
    }
}

// rank of (vc, ic) among the nr re-scored candidates by (value descending, feature ascending)
__device__ __forceinline__ uint32_t enc_rank(const float* val, const int32_t* idx, uint32_t nr, float vc, int32_t ic) {
    uint32_t rank = 0;
    for (uint32_t o = 0; o < nr; ++o) {
        const float vo = val[o];
        rank += (vo > vc) || (vo == vc && idx[o] < ic);
    }
    return rank;
}
