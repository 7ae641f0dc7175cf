// Everything of the SAE that runs between one step and the next (C ABI: pv_sae_apply, pv_sae_renorm_decoder, pv_sae_sync_shadows,
// pv_sae_grad_sqnorm* in include/pv_native.h): the clip norm, clip -> project -> Adam fused per tensor, the decoder renorm, the encoder
// shadows.  The steps that produce the gradients: sae.hip, sae_dense.hip, sae_gated.hip, sae_gated_topk.hip, sae_tp.hip.
//
// W_enc lives three times: the module's parameter W [d_in][d_sae]; WT = its transpose [d_sae][d_in] in fp32 -- the
// layout the sparse backward writes gradients in and the exact re-scoring of sae_enc.hip gathers rows from, hence
// the layout Adam runs in (gradient, both moments and WT are read and written coalesced, feature rows [j_lo, j_hi) are
// contiguous: the data-parallel trainer shards the optimizer by feature); and W16T = WT rounded to fp16, the B operand of
// the filter GEMM.  One workgroup of wenc_rows_kernel owns 32 features x all d_in: tile-wise it updates WT / moments / W16T in place,
// transposes the new values through LDS into W, and leaves ||W_enc[:, j]||^2 (the filter's error bound) in colsq.
// MODE 0: Adam step.  MODE 1: rebuild W, W16T, colsq from WT (after an all-gather of WT).  MODE 2: rebuild WT, W16T,
// colsq from W (parameters edited from outside).
#include <math.h>

#include "sae_bwd.hpp"

namespace {

// The optimizer state (both Adam moments, 302 MB) and the gradients are touched ONCE per step: streamed past the caches
// (nontemporal), so that what the next step gathers by row -- W_dec, W_enc^T and its fp16 copy, 188 MB, written by the same
// kernels -- is what stays in the 256 MB MALL.  -DPV_NO_NT (A/B builds): plain accesses.
typedef float pv_f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld4_stream(const float* p, bool ok) {
#ifdef PV_NO_NT
    return ld4(p, ok);
#else
    if (!ok) return make_float4(0.f, 0.f, 0.f, 0.f);
    const pv_f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const pv_f32x4*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
#endif
}
__device__ __forceinline__ float ld1_stream(const float* p) {
#ifdef PV_NO_NT
    return *p;
#else
    return __builtin_nontemporal_load(p);
#endif
}
__device__ __forceinline__ void st1_stream(float* p, float v) {
#ifdef PV_NO_NT
    *p = v;
#else
    __builtin_nontemporal_store(v, p);
#endif
}
__device__ __forceinline__ void st4_stream(float* p, const float4& v) {
#ifdef PV_NO_NT
    *reinterpret_cast<float4*>(p) = v;
#else
    __builtin_nontemporal_store(pv_f32x4{v.x, v.y, v.z, v.w}, reinterpret_cast<pv_f32x4*>(p));
#endif
}

// clip norm from the per-feature terms of the backward (+ gb_dec): one workgroup, fixed summation order
__global__ __launch_bounds__(1024) void sqnorm_rowsq_kernel(const float* __restrict__ rowsq, int d_sae, const float* __restrict__ gb_dec,
                                                            int d_in, float* __restrict__ scalars, const float* __restrict__ extra0,
                                                            int n0, const float* __restrict__ extra1, int n1) {
    __shared__ float red[16];
    float s = 0.f;
#pragma unroll 8
    for (int j = threadIdx.x; j < d_sae; j += 1024) s += rowsq[j];             // (8 loads in flight; the sum in order)
    for (int i = threadIdx.x; i < d_in; i += 1024) s += gb_dec[i] * gb_dec[i];
    for (int i = threadIdx.x; i < n0; i += 1024) s += extra0[i] * extra0[i];          // transcoder: gb_dec_out, gW_skip
    for (int i = threadIdx.x; i < n1; i += 1024) s += extra1[i] * extra1[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int w = 0; w < 16; ++w) t += red[w];
        scalars[3] = t;
    }
}

// ------------------------------------------------------------------------------------------------
// gradient square-norm (two stage, deterministic)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sqnorm_partial_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ partial) {
    __shared__ float red[4];
    float s = 0.f;
    for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (int64_t)gridDim.x * 1024) {
        if (i + 3 < n) {
            const float4 v = *reinterpret_cast<const float4*>(g + i);
            s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        } else {
            for (int64_t t = i; t < n; ++t) s += g[t] * g[t];
        }
    }
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// ------------------------------------------------------------------------------------------------
// apply: clip -> project -> Adam  (train_sae.py:394-401; sae.py:279-297; torch.optim.Adam defaults)
// ------------------------------------------------------------------------------------------------
struct AdamC {
    float lr, b1, b2, eps, bc1, bc2_sqrt, max_norm;
};
__device__ __forceinline__ float clip_coef(const float* scalars, float max_norm) {
    if (max_norm <= 0.f) return 1.f;
    const float total = sqrtf(scalars[3]);
    return fminf(max_norm / (total + 1e-6f), 1.f);          // clip_grad_norm_: clamp(max_norm/(norm+1e-6), max=1)
}
__device__ __forceinline__ float adam_update(float w, float g, float& m, float& v, const AdamC& c) {
    m = m + (g - m) * (1.f - c.b1);                         // exp_avg.lerp_(grad, 1 - beta1)
    v = v * c.b2 + (1.f - c.b2) * g * g;                    // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1-beta2)
    const float denom = sqrtf(v) / c.bc2_sqrt + c.eps;
    return w - (c.lr / c.bc1) * (m / denom);
}

// two vectors in one launch (b_enc's feature range and b_dec): blocks [0, nb0) take the first
struct AdamVec2 {
    float* W0; const float* G0; float* M0; float* V0; int lo0, hi0, nb0;
    float* W1; const float* G1; float* M1; float* V1; int hi1;
};
__device__ __forceinline__ void adam_vec2_body(int bid, const AdamVec2& a, const float* __restrict__ scalars, const AdamC& c) {
    const bool first = bid < a.nb0;
    const int i = first ? a.lo0 + bid * 256 + threadIdx.x : (bid - a.nb0) * 256 + threadIdx.x;
    if (i >= (first ? a.hi0 : a.hi1)) return;
    float* W = first ? a.W0 : a.W1;
    const float* G = first ? a.G0 : a.G1;
    float* M = first ? a.M0 : a.M1;
    float* V = first ? a.V0 : a.V1;
    const float coef = clip_coef(scalars, c.max_norm);
    float m = M[i], v = V[i];
    W[i] = adam_update(W[i], G[i] * coef, m, v, c);
    M[i] = m;
    V[i] = v;
}
__global__ __launch_bounds__(256) void adam_vec2_kernel(const AdamVec2 a, const float* __restrict__ scalars, AdamC c) {
    adam_vec2_body(blockIdx.x, a, scalars, c);
}

template <int V4>   // W_dec rows [j_lo, j_hi): one wave per row (16 bytes per lane and load), with the parallel-gradient projection
__global__ __launch_bounds__(256) void adam_wdec_kernel(float* __restrict__ W, const float* __restrict__ G,
                                                        float* __restrict__ M, float* __restrict__ V,
                                                        const float* __restrict__ scalars, AdamC c, int j_lo, int j_hi, int d,
                                                        const float* inv_norm, float* inv_next /* may be the same array */,
                                                        const uint32_t* __restrict__ live_offs) {
    const int lane = threadIdx.x & 63;
    const int j = j_lo + blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= j_hi) return;
    const bool live = !live_offs || live_offs[j + 1] != live_offs[j];        // (wave-uniform) PV_SAE_SPARSE_GRADS: no pair, g = 0
    const float coef = clip_coef(scalars, c.max_norm);
    const float rn = inv_norm ? inv_norm[j] : 1.f;            // pending set_decoder_norm_to_unit_norm (see pv_sae_step)
    float4 w[V4], g[V4], m[V4], v[V4];
    bool ok[V4];
    float dot = 0.f;
#pragma unroll
    for (int i = 0; i < V4; ++i) {
        const int col = 4 * lane + 256 * i;
        ok[i] = col < d;
        const int64_t o = (int64_t)j * d + col;
        w[i] = ld4(W + o, ok[i]);
        g[i] = ld4_stream(G + o, ok[i] && live);
        m[i] = ld4_stream(M + o, ok[i]);
        v[i] = ld4_stream(V + o, ok[i]);
    }
#pragma unroll
    for (int i = 0; i < V4; ++i) {
        w[i].x *= rn; w[i].y *= rn; w[i].z *= rn; w[i].w *= rn;
        g[i].x *= coef; g[i].y *= coef; g[i].z *= coef; g[i].w *= coef;
        dot += g[i].x * w[i].x + g[i].y * w[i].y + g[i].z * w[i].z + g[i].w * w[i].w;
    }
    dot = wave_sum(dot);
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < V4; ++i) {
        if (!ok[i]) continue;
        const int64_t o = (int64_t)j * d + 4 * lane + 256 * i;
        float4 wn;                                          // g - dot * w: remove_gradient_parallel_to_decoder_directions
        wn.x = adam_update(w[i].x, g[i].x - dot * w[i].x, m[i].x, v[i].x, c);
        wn.y = adam_update(w[i].y, g[i].y - dot * w[i].y, m[i].y, v[i].y, c);
        wn.z = adam_update(w[i].z, g[i].z - dot * w[i].z, m[i].z, v[i].z, c);
        wn.w = adam_update(w[i].w, g[i].w - dot * w[i].w, m[i].w, v[i].w, c);
        *reinterpret_cast<float4*>(W + o) = wn;
        st4_stream(M + o, m[i]);
        st4_stream(V + o, v[i]);
        sq += wn.x * wn.x + wn.y * wn.y + wn.z * wn.z + wn.w * wn.w;
    }
    // the next step's set_decoder_norm_to_unit_norm needs 1 / ||row|| of what was just written: leave it behind
    // (PV_SAE_INV_NORM_VALID) instead of re-reading W_dec for it
    if (inv_next) {
        sq = wave_sum(sq);
        if (lane == 0) inv_next[j] = 1.0f / sqrtf(sq);
    }
}

// W_enc's Adam step when the parameter's own [d_in][d_sae] layout is NOT rewritten (lazy materialisation, pv_sae_state.W_enc ==
// NULL): everything lives in the transposed domain -- the fp32 master WT, gradient, moments, the fp16 shadow and the column
// norms are all [d_sae][d_in] rows -- so this is the row-streaming form of adam_wdec_kernel (a wave per feature row, 16 bytes
// per lane and load, no LDS transposes) instead of the 32 x 64 tile walk of wenc_rows_kernel.  Same arithmetic per element.
template <int V4>
__global__ __launch_bounds__(256) void adam_wenct_kernel(float* __restrict__ WT, _Float16* __restrict__ W16T, float* __restrict__ colsq,
                                                         const float* __restrict__ GT, float* __restrict__ MT, float* __restrict__ VT,
                                                         const float* __restrict__ scalars, AdamC c, int j_lo, int j_hi, int d,
                                                         const uint32_t* __restrict__ live_offs, int nb_rows, const AdamVec2 v2) {
    // workgroups beyond nb_rows (v2.nb0 + the blocks of b_dec of them): the two bias vectors' Adam (adam_vec2_body) -- it was a launch
    if ((int)blockIdx.x >= nb_rows) {
        adam_vec2_body(blockIdx.x - nb_rows, v2, scalars, c);
        return;
    }
    const int lane = threadIdx.x & 63;
    const int j = j_lo + blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= j_hi) return;
    const bool live = !live_offs || live_offs[j + 1] != live_offs[j];        // (wave-uniform) PV_SAE_SPARSE_GRADS: no pair, g = 0
    const float coef = clip_coef(scalars, c.max_norm);
    float4 w[V4], g[V4], m[V4], v[V4];
    bool ok[V4];
#pragma unroll
    for (int i = 0; i < V4; ++i) {
        const int col = 4 * lane + 256 * i;
        ok[i] = col < d;
        const int64_t o = (int64_t)j * d + col;
        w[i] = ld4(WT + o, ok[i]);
        g[i] = ld4_stream(GT + o, ok[i] && live);
        m[i] = ld4_stream(MT + o, ok[i]);
        v[i] = ld4_stream(VT + o, ok[i]);
    }
    float sq = 0.f;
    bool big = false;
#pragma unroll
    for (int i = 0; i < V4; ++i) {
        if (!ok[i]) continue;
        const int64_t o = (int64_t)j * d + 4 * lane + 256 * i;
        float4 wn;
        wn.x = adam_update(w[i].x, g[i].x * coef, m[i].x, v[i].x, c);
        wn.y = adam_update(w[i].y, g[i].y * coef, m[i].y, v[i].y, c);
        wn.z = adam_update(w[i].z, g[i].z * coef, m[i].z, v[i].z, c);
        wn.w = adam_update(w[i].w, g[i].w * coef, m[i].w, v[i].w, c);
        *reinterpret_cast<float4*>(WT + o) = wn;
        st4_stream(MT + o, m[i]);
        st4_stream(VT + o, v[i]);
        typedef _Float16 h4 __attribute__((ext_vector_type(4)));
        const h4 hv = {(_Float16)wn.x, (_Float16)wn.y, (_Float16)wn.z, (_Float16)wn.w};
        *reinterpret_cast<h4*>(W16T + o) = hv;
        sq += wn.x * wn.x + wn.y * wn.y + wn.z * wn.z + wn.w * wn.w;
        big = big || !(fabsf(wn.x) <= 6.0e4f) || !(fabsf(wn.y) <= 6.0e4f) || !(fabsf(wn.z) <= 6.0e4f) || !(fabsf(wn.w) <= 6.0e4f);
    }
    sq = wave_sum(sq);
    const bool any_big = __any(big);                        // outside the fp16 range (or NaN): the filter must not be trusted
    if (lane == 0) colsq[j] = any_big ? INFINITY : sq;
}

// the tile walk over W_enc's three copies (the file header); MODE 0: Adam, 1: from WT, 2: from W
template <int MODE>
__global__ __launch_bounds__(256) void wenc_rows_kernel(float* __restrict__ W, float* __restrict__ WT, _Float16* __restrict__ W16T,
                                                        float* __restrict__ colsq, const float* __restrict__ GT,
                                                        float* __restrict__ MT, float* __restrict__ VT,
                                                        const float* __restrict__ scalars, AdamC c, int d_in, int d_sae,
                                                        int j_lo, int j_hi, const uint32_t* __restrict__ live_offs = nullptr) {
    constexpr int NC = 2;                                     // 32-column chunks per iteration (16 independent loads per array)
    __shared__ float tile[NC][32][33];
    const int j0 = j_lo + blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    float coef = 1.f;
    if constexpr (MODE == 0) coef = clip_coef(scalars, c.max_norm);
    float sq[4] = {0.f, 0.f, 0.f, 0.f};
    bool big = false;
    bool live[4] = {true, true, true, true};                  // PV_SAE_SPARSE_GRADS: rows of features without a pair are not read
    if constexpr (MODE == 0) {
        if (live_offs) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = j0 + ty + 8 * r;
                live[r] = j < j_hi && live_offs[j + 1] != live_offs[j];
            }
        }
    }
    for (int i0 = 0; i0 < d_in; i0 += 32 * NC) {
        if constexpr (MODE == 2) {
#pragma unroll
            for (int u = 0; u < NC; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) {                   // read W[i][j0 + tx] coalesced along j
                    const int i = i0 + 32 * u + ty + 8 * r, j = j0 + tx;
                    tile[u][tx][ty + 8 * r] = (i < d_in && j < j_hi) ? W[(int64_t)i * d_sae + j] : 0.f;
                }
            __syncthreads();
        }
        float wv[NC][4], gv[NC][4], mv[NC][4], vv[NC][4];
        if constexpr (MODE == 0) {
#pragma unroll
            for (int u = 0; u < NC; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = j0 + ty + 8 * r, i = i0 + 32 * u + tx;
                    const bool in = j < j_hi && i < d_in;
                    const int64_t o = (int64_t)j * d_in + i;
                    wv[u][r] = in ? WT[o] : 0.f;
                    gv[u][r] = (in && live[r]) ? ld1_stream(GT + o) : 0.f;      // (optimizer state and gradients: streamed, see ld4_stream)
                    mv[u][r] = in ? ld1_stream(MT + o) : 0.f;
                    vv[u][r] = in ? ld1_stream(VT + o) : 0.f;
                }
        }
#pragma unroll
        for (int u = 0; u < NC; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = j0 + ty + 8 * r, i = i0 + 32 * u + tx;
                if (j < j_hi && i < d_in) {
                    const int64_t o = (int64_t)j * d_in + i;
                    float wn;
                    if constexpr (MODE == 0) {
                        float m = mv[u][r], v = vv[u][r];
                        wn = adam_update(wv[u][r], gv[u][r] * coef, m, v, c);
                        st1_stream(MT + o, m);
                        st1_stream(VT + o, v);
                        WT[o] = wn;
                    } else if constexpr (MODE == 1) {
                        wn = WT[o];
                    } else {
                        wn = tile[u][ty + 8 * r][tx];
                        WT[o] = wn;
                    }
                    W16T[o] = (_Float16)wn;
                    sq[r] += wn * wn;
                    big = big || !(fabsf(wn) <= 6.0e4f);        // outside the fp16 range (or NaN): the filter must not be trusted
                    if constexpr (MODE != 2) { if (W) tile[u][ty + 8 * r][tx] = wn; }
                }
            }
        if constexpr (MODE != 2) {
            if (W) {                                                   // (uniform) W == nullptr: the parameter layout is materialised lazily
                __syncthreads();
#pragma unroll
                for (int u = 0; u < NC; ++u)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i = i0 + 32 * u + ty + 8 * r, j = j0 + tx;
                        if (i < d_in && j < j_hi) W[(int64_t)i * d_sae + j] = tile[u][tx][ty + 8 * r];
                    }
                __syncthreads();
            }
        } else {
            __syncthreads();
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float s = big ? INFINITY : sq[r];
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);           // the 32 lanes that share ty
        const int j = j0 + ty + 8 * r;
        if (tx == 0 && j < j_hi) colsq[j] = s;
    }
}

__global__ __launch_bounds__(256) void adam_vec_kernel(float* __restrict__ W, const float* __restrict__ G,
                                                       float* __restrict__ M, float* __restrict__ V,
                                                       const float* __restrict__ scalars, AdamC c, int lo, int hi) {
    const int i = lo + blockIdx.x * 256 + threadIdx.x;
    if (i >= hi) return;
    const float coef = clip_coef(scalars, c.max_norm);
    float m = M[i], v = V[i];
    W[i] = adam_update(W[i], G[i] * coef, m, v, c);
    M[i] = m;
    V[i] = v;
}

// set_decoder_norm_to_unit_norm (sae.py:275-277)
template <int DPL>
__global__ __launch_bounds__(256) void renorm_rows_kernel(float* __restrict__ W, int rows, int d) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= rows) return;
    float w[DPL];
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < DPL; ++i) {
        const int c = lane + 64 * i;
        w[i] = c < d ? W[(int64_t)j * d + c] : 0.f;
        sq += w[i] * w[i];
    }
    const float nrm = sqrtf(wave_sum(sq));
#pragma unroll
    for (int i = 0; i < DPL; ++i) {
        const int c = lane + 64 * i;
        if (c < d) W[(int64_t)j * d + c] = w[i] / nrm;
    }
}

}  // namespace

#define DPL_DISPATCH(d_in, CALL)            \
    do {                                    \
        if ((d_in) <= 64 * 4) { CALL(4); }  \
        else if ((d_in) <= 64 * 12) { CALL(12); } \
        else if ((d_in) <= 64 * 16) { CALL(16); } \
        else { CALL(20); }                  \
    } while (0)

extern "C" int pv_sae_renorm_decoder(pv_sae_plan* plan, pv_sae_state* st, void* stream_) {
    PV_REQUIRE(plan && st && st->W_dec, "null argument");
    hipStream_t stream = (hipStream_t)stream_;
    const pv_sae_desc& d = plan->d;
    const dim3 grid((d.d_sae + 3) / 4), block(256);
#define CALL(D) hipLaunchKernelGGL((renorm_rows_kernel<D>), grid, block, 0, stream, st->W_dec, d.d_sae, d.d_in)
    DPL_DISPATCH(d.d_in, CALL);
#undef CALL
    PV_LAUNCH_CHECK("renorm_rows_kernel");
    plan->renorm_pending = false;
    return PV_OK;
}

// Rebuild the encoder shadows for features [j_lo, j_hi).  from_transposed = 0: W_enc is the truth (parameters were edited
// outside: load_state_dict, a fresh engine) -> W_encT, W_enc16T, enc_colsq; 1: W_encT is the truth (an all-gather of the
// sharded optimizer's slices just landed) -> W_enc, W_enc16T, enc_colsq.
extern "C" int pv_sae_sync_shadows(pv_sae_plan* plan, pv_sae_state* st, int32_t from_transposed, int32_t j_lo, int32_t j_hi,
                                   void* stream_) {
    PV_REQUIRE(plan && st && st->W_enc && st->W_encT && st->W_enc16T && st->enc_colsq, "null argument");
    const pv_sae_desc& d = plan->d;
    PV_REQUIRE(j_lo >= 0 && j_lo <= j_hi && j_hi <= d.d_sae, "feature range");
    if (j_lo == j_hi) return PV_OK;
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid((j_hi - j_lo + 31) / 32), block(256);
    const auto rebuild = from_transposed ? wenc_rows_kernel<1> : wenc_rows_kernel<2>;
    hipLaunchKernelGGL(rebuild, grid, block, 0, stream, st->W_enc, st->W_encT, (_Float16*)st->W_enc16T, st->enc_colsq,
                       (const float*)nullptr, (float*)nullptr, (float*)nullptr, (const float*)nullptr, AdamC{}, d.d_in, d.d_sae, j_lo, j_hi,
                       (const uint32_t*)nullptr);
    PV_LAUNCH_CHECK("wenc_rows_kernel");
    return PV_OK;
}

// the clip norm from the per-feature terms the last pv_sae_step left in its workspace
extern "C" int pv_sae_grad_sqnorm_step(pv_sae_plan* plan, const pv_sae_state* st, const void* workspace, float* scalars, void* stream_) {
    PV_REQUIRE(plan && st && workspace && scalars && st->gb_dec, "null argument");
    const pv_sae_desc& d = plan->d;
    const SaeWs ws = sae_carve(d);
    const bool tc = sae_is_tc(st);
    PV_REQUIRE(!tc || st->tc.gb_dec_out, "transcoder state");
    hipLaunchKernelGGL(sqnorm_rowsq_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream_,
                       (const float*)((const unsigned char*)workspace + ws.rowsq), d.d_sae, (const float*)st->gb_dec, d.d_in, scalars,
                       tc ? (const float*)st->tc.gb_dec_out : (const float*)nullptr, tc ? d.d_in : 0,
                       (tc && st->tc.gW_skip) ? (const float*)st->tc.gW_skip : (const float*)nullptr,
                       (tc && st->tc.gW_skip) ? d.d_in * d.d_in : 0);
    PV_LAUNCH_CHECK("sqnorm_rowsq_kernel");
    return PV_OK;
}

// sum of squares of a flat gradient buffer -> scalars[3]; `partial` = 1024 floats of scratch
extern "C" int pv_sae_grad_sqnorm(const float* flat_grads, int64_t n, float* partial, float* scalars, void* stream_) {
    PV_REQUIRE(flat_grads && partial && scalars && n > 0, "null argument");
    PV_REQUIRE(pv_aligned16(flat_grads), "gradient buffer must be 16-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(sqnorm_partial_kernel, dim3(1024), dim3(256), 0, stream, flat_grads, n, partial);
    sae_reduce_sum(partial, scalars, 1024, 1.0f, 3, -1, stream);
    PV_LAUNCH_CHECK("sqnorm kernels");
    return PV_OK;
}

// The same over the gradient rows of features [j_lo, j_hi) only (gW_enc^T, gW_dec, gb_enc slices; + gb_dec when
// include_b_dec): the local term of the sharded optimizer's clip norm (the ranks' terms are summed by one scalar all-reduce).
extern "C" int pv_sae_grad_sqnorm_rows(pv_sae_plan* plan, const pv_sae_state* st, int32_t j_lo, int32_t j_hi, int32_t include_b_dec,
                                       float* partial, float* scalars, void* stream_) {
    PV_REQUIRE(plan && st && partial && scalars && st->gW_enc && st->gW_dec && st->gb_enc && st->gb_dec, "null argument");
    const pv_sae_desc& d = plan->d;
    PV_REQUIRE(j_lo >= 0 && j_lo <= j_hi && j_hi <= d.d_sae, "feature range");
    hipStream_t stream = (hipStream_t)stream_;
    PV_HIP_CHECK(hipMemsetAsync(partial, 0, 1024 * 4, stream));
    const int64_t nrow = (int64_t)(j_hi - j_lo) * d.d_in;
    if (nrow > 0) {
        PV_REQUIRE(((int64_t)j_lo * d.d_in) % 4 == 0, "slice must start on a 16-byte boundary");
        hipLaunchKernelGGL(sqnorm_partial_kernel, dim3(384), dim3(256), 0, stream, (const float*)st->gW_enc + (int64_t)j_lo * d.d_in, nrow, partial);
        hipLaunchKernelGGL(sqnorm_partial_kernel, dim3(384), dim3(256), 0, stream, (const float*)st->gW_dec + (int64_t)j_lo * d.d_in, nrow, partial + 384);
        hipLaunchKernelGGL(sqnorm_partial_kernel, dim3(8), dim3(256), 0, stream, (const float*)st->gb_enc + j_lo, (int64_t)(j_hi - j_lo), partial + 768);
    }
    if (include_b_dec)
        hipLaunchKernelGGL(sqnorm_partial_kernel, dim3(8), dim3(256), 0, stream, (const float*)st->gb_dec, (int64_t)d.d_in, partial + 776);
    sae_reduce_sum(partial, scalars, 1024, 1.0f, 3, -1, stream);
    PV_LAUNCH_CHECK("sqnorm kernels");
    return PV_OK;
}

extern "C" int pv_sae_apply(pv_sae_plan* plan, pv_sae_state* st, const float* scalars, float max_grad_norm, float lr,
                            int32_t step, int32_t j_lo, int32_t j_hi, void* stream_) {
    PV_REQUIRE(plan && st && scalars && step >= 1, "null argument / step must be >= 1");
    PV_REQUIRE(st->mW_enc && st->mW_dec && st->mb_enc && st->mb_dec && st->vW_enc && st->vW_dec && st->vb_enc && st->vb_dec, "Adam state");
    PV_REQUIRE(st->W_encT && st->W_enc16T && st->enc_colsq, "encoder shadows");
    hipStream_t stream = (hipStream_t)stream_;
    const pv_sae_desc& d = plan->d;
    PV_REQUIRE(j_lo >= 0 && j_lo <= j_hi && j_hi <= d.d_sae, "feature range");
    // (every check stands in front of the first launch: a call that returns an error has not touched the state)
    if (sae_is_tc(st)) {
        const pv_sae_transcoder& t = st->tc;
        PV_REQUIRE(t.gb_dec_out && t.mb_dec_out && t.vb_dec_out && (!t.W_skip || (t.gW_skip && t.mW_skip && t.vW_skip)), "transcoder Adam state");
    }
    if (sae_is_gated(st)) {
        const pv_sae_gated& t = st->gt;
        PV_REQUIRE(t.r_mag && t.b_mag && t.gb_gate && t.gr_mag && t.gb_mag && t.mb_gate && t.mr_mag && t.mb_mag && t.vb_gate && t.vr_mag && t.vb_mag,
                   "gated Adam state");
        PV_REQUIRE(j_lo == 0 && j_hi == d.d_sae, "gated SAE: the whole feature range");
    }
    AdamC c;
    c.lr = lr; c.b1 = 0.9f; c.b2 = 0.999f; c.eps = 1e-8f; c.max_norm = max_grad_norm;
    c.bc1 = (float)(1.0 - pow(0.9, (double)step));
    c.bc2_sqrt = (float)sqrt(1.0 - pow(0.999, (double)step));
    const int nj = j_hi - j_lo;
    // algorithmic bytes: 7 x 4 per parameter (w, g, m, v read; w, m, v written) + the two extra copies of W_enc (fp32 + fp16)
    ProfScope prof(PV_PROF_SAE_APPLY, stream, 0.0, 7.0 * 4.0 * (2.0 * d.d_in * (double)nj + nj + d.d_in) + 6.0 * d.d_in * (double)nj);
    const dim3 block(256);
    AdamVec2 v2;
    v2.W0 = st->b_enc; v2.G0 = (const float*)st->gb_enc; v2.M0 = st->mb_enc; v2.V0 = st->vb_enc; v2.lo0 = j_lo; v2.hi0 = j_hi;
    v2.nb0 = (nj + 255) / 256; v2.W1 = st->b_dec; v2.G1 = (const float*)st->gb_dec; v2.M1 = st->mb_dec; v2.V1 = st->vb_dec; v2.hi1 = d.d_in;
    bool vec2_done = false;
    if (nj > 0) {
        const float* inv_norm = plan->renorm_pending ? (const float*)st->dec_inv_norm : nullptr;
#define CALL(D) hipLaunchKernelGGL((adam_wdec_kernel<D>), dim3((nj + 3) / 4), block, 0, stream, st->W_dec, (const float*)st->gW_dec, st->mW_dec, st->vW_dec, scalars, c, j_lo, j_hi, d.d_in, inv_norm, st->dec_inv_norm, plan->live_offs)
        V4_DISPATCH(d.d_in, CALL);
#undef CALL
        if (st->W_enc) {
            hipLaunchKernelGGL((wenc_rows_kernel<0>), dim3((nj + 31) / 32), block, 0, stream, st->W_enc, st->W_encT, (_Float16*)st->W_enc16T,
                               st->enc_colsq, (const float*)st->gW_enc, st->mW_enc, st->vW_enc, scalars, c, d.d_in, d.d_sae, j_lo, j_hi,
                               plan->live_offs);
        } else {                                                  // lazy parameter layout: everything stays in the transposed domain
            // (the two bias vectors ride at the end of this launch)
            vec2_done = g_pv_tuning.sae_fold != 0;
            const int nb_rows = (nj + 3) / 4, nb_v2 = vec2_done ? v2.nb0 + (d.d_in + 255) / 256 : 0;
#define CALL(D) hipLaunchKernelGGL((adam_wenct_kernel<D>), dim3(nb_rows + nb_v2), block, 0, stream, st->W_encT, (_Float16*)st->W_enc16T, st->enc_colsq, (const float*)st->gW_enc, st->mW_enc, st->vW_enc, scalars, c, j_lo, j_hi, d.d_in, plan->live_offs, nb_rows, v2)
            V4_DISPATCH(d.d_in, CALL);
#undef CALL
        }
    }
    if (!vec2_done)     // b_enc's feature range and b_dec: one launch
        hipLaunchKernelGGL(adam_vec2_kernel, dim3(v2.nb0 + (d.d_in + 255) / 256), block, 0, stream, v2, scalars, c);
    if (sae_is_tc(st)) {                                               // transcoder: plain Adam on the decoder's own bias and the skip matrix
        const pv_sae_transcoder& t = st->tc;
        hipLaunchKernelGGL(adam_vec_kernel, dim3((d.d_in + 255) / 256), block, 0, stream, t.b_dec_out, (const float*)t.gb_dec_out,
                           t.mb_dec_out, t.vb_dec_out, scalars, c, 0, d.d_in);
        if (t.W_skip)
            hipLaunchKernelGGL(adam_vec_kernel, dim3((d.d_in * d.d_in + 255) / 256), block, 0, stream, t.W_skip, (const float*)t.gW_skip,
                               t.mW_skip, t.vW_skip, scalars, c, 0, d.d_in * d.d_in);
    }
    if (sae_is_gated(st)) {                                            // gated SAE: plain Adam on b_gate, r_mag, b_mag
        const pv_sae_gated& t = st->gt;
        const dim3 gv((d.d_sae + 255) / 256);
        hipLaunchKernelGGL(adam_vec_kernel, gv, block, 0, stream, t.b_gate, (const float*)t.gb_gate, t.mb_gate, t.vb_gate, scalars, c, 0, d.d_sae);
        hipLaunchKernelGGL(adam_vec_kernel, gv, block, 0, stream, t.r_mag, (const float*)t.gr_mag, t.mr_mag, t.vr_mag, scalars, c, 0, d.d_sae);
        hipLaunchKernelGGL(adam_vec_kernel, gv, block, 0, stream, t.b_mag, (const float*)t.gb_mag, t.mb_mag, t.vb_mag, scalars, c, 0, d.d_sae);
    }
    PV_LAUNCH_CHECK("adam kernels");
    if (j_lo == 0 && j_hi == d.d_sae) plan->renorm_pending = false;      // (a sharded apply leaves the other ranks' rows to the all-gather)
    return PV_OK;
}
