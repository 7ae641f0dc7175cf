// ------------------------------------------------------------------------------------------------
// Gated SAE step (GatedSparseAutoencoder, sae.py:648-792; pv_sae_gated).  hs [2N][F]: rows [0, N) feature_acts (later dM, then
// dP), rows [N, 2N) relu(gate pre-activation) (later dG); dYs [2N][D]: rows [0, N) dY of the reconstruction, rows [N, 2N)
// d aux / d (reconstruction through the gate).  Stacking the two row sets makes the two decoder products one GEMM, and
// gW_dec = f^T dY + relu(gate)^T dVia one GEMM over K = 2N (sae_dense_gemm.hip).  The sparse form: below; the top-k form: sae_gated_topk.hip.
// ------------------------------------------------------------------------------------------------
#include <algorithm>
#include "sae_bwd.hpp"
#include "sae_dense_gemm.hpp"

namespace {
struct GatedWs {
    size_t total, hs, dys, kpart, colpart2, auxpart, vec0, vec1, vec2, tmpd, cspart;
};
GatedWs gated_carve(const pv_sae_desc& d, int N) {
    GatedWs w;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (size_t)pv_align_up((int64_t)bytes, 256); return o; };
    const size_t F = d.d_sae, D = d.d_in, n = N;
    w.hs = take(2 * n * F * 4);
    w.dys = take(2 * n * D * 4);
    w.kpart = take((size_t)PV_SAE_DENSE_SPLITK * 2 * n * D * 4);
    w.colpart2 = take(((n + 63) / 64) * F * 4);
    w.auxpart = take(n * 4);
    w.vec0 = take(F * 4);
    w.vec1 = take(F * 4);
    w.vec2 = take(F * 4);
    w.tmpd = take(D * 4);
    w.cspart = take((n / 16 + 2) * D * 4);
    w.total = off + 256;
    return w;
}

// rows [0, N): decoder output -> LN-out, mse partial, dY (as dense_finish_kernel); rows [N, 2N): reconstruction through the gate
// -> auxiliary loss partial and its gradient (sae.py:786-792: sum_i (via - sae_in)^2, mean over the batch).  One wave per row.
__global__ __launch_bounds__(256) void gated_finish_kernel(const float* __restrict__ x, const float* __restrict__ sae_in,
                                                           const float* __restrict__ kpart, int splits, int64_t zstride,
                                                           const float* __restrict__ b_dec, const float* __restrict__ mu,
                                                           const float* __restrict__ sd, const float* __restrict__ norm,
                                                           float* __restrict__ sae_out, float* __restrict__ dYs,
                                                           float* __restrict__ loss_partial, float* __restrict__ aux_partial, int n_tok,
                                                           int d, float grad_scale, float aux_scale /* 2 / N */,
                                                           const uint32_t* __restrict__ gate, uint32_t* __restrict__ amax = nullptr) {
    // amax (or NULL): partial maxima of |dYs| (DG_AMAX_SLOTS words, see DenseGemm.a_max)
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gate && *gate != 1u) return;                           // (gate: as in DenseGemm)
    if (r >= 2 * n_tok) return;
    float gmax = 0.f;
    const bool second = r >= n_tok;
    const int n = second ? r - n_tok : r;
    const float m = mu[n], sdv = sd[n], nf = norm[n];
    float lsum = 0.f;
    for (int c = 4 * lane; c < d; c += 256) {
        float4 a = *reinterpret_cast<const float4*>(kpart + (int64_t)r * d + c);
        for (int z = 1; z < splits; ++z) {
            const float4 t = *reinterpret_cast<const float4*>(kpart + z * zstride + (int64_t)r * d + c);
            a.x += t.x; a.y += t.y; a.z += t.z; a.w += t.w;
        }
        const float4 bd = *reinterpret_cast<const float4*>(b_dec + c);
        float4 e, g;
        if (!second) {
            const float4 xv = *reinterpret_cast<const float4*>(x + (int64_t)n * d + c);
            float4 o;
            o.x = (a.x + bd.x) * sdv + m; o.y = (a.y + bd.y) * sdv + m; o.z = (a.z + bd.z) * sdv + m; o.w = (a.w + bd.w) * sdv + m;
            e.x = o.x - xv.x; e.y = o.y - xv.y; e.z = o.z - xv.z; e.w = o.w - xv.w;
            if (sae_out) *reinterpret_cast<float4*>(sae_out + (int64_t)n * d + c) = o;
            lsum += (e.x * e.x) / nf + (e.y * e.y) / nf + (e.z * e.z) / nf + (e.w * e.w) / nf;
            g.x = grad_scale * e.x / nf * sdv; g.y = grad_scale * e.y / nf * sdv;
            g.z = grad_scale * e.z / nf * sdv; g.w = grad_scale * e.w / nf * sdv;
        } else {
            const float4 sv = *reinterpret_cast<const float4*>(sae_in + (int64_t)n * d + c);
            e.x = a.x + bd.x - sv.x; e.y = a.y + bd.y - sv.y; e.z = a.z + bd.z - sv.z; e.w = a.w + bd.w - sv.w;
            lsum += e.x * e.x + e.y * e.y + e.z * e.z + e.w * e.w;
            g.x = aux_scale * e.x; g.y = aux_scale * e.y; g.z = aux_scale * e.z; g.w = aux_scale * e.w;
        }
        *reinterpret_cast<float4*>(dYs + (int64_t)r * d + c) = g;
        gmax = fmaxf(fmaxf(gmax, fmaxf(fabsf(g.x), fabsf(g.y))), fmaxf(fabsf(g.z), fabsf(g.w)));
    }
    lsum = wave_sum(lsum);
    if (lane == 0) (second ? aux_partial : loss_partial)[n] = lsum;
    if (amax) {
        gmax = wave_max(gmax);
        if (lane == 0) atomicMax(amax + (r & (DG_AMAX_SLOTS - 1)), __float_as_uint(gmax));
    }
}

// scalars[0] = mse + l1 + aux (sae.py:748), one thread
__global__ void gated_loss_kernel(float* __restrict__ scalars, const uint32_t* __restrict__ gate) {
    if (gate && *gate != 1u) return;
    scalars[0] = scalars[1] + scalars[4] + scalars[6];
}

// dP = dM e^r + dG, in place over dM (rows [0, N) of hs; dG = rows [N, 2N))
// amax (or NULL): partial maxima of |dP| (DG_AMAX_SLOTS words, see DenseGemm.a_max)
__global__ __launch_bounds__(256) void gated_dp_kernel(float* __restrict__ hs, const float* __restrict__ r_mag, int64_t n_rows, int F,
                                                       const uint32_t* __restrict__ gate, uint32_t* __restrict__ amax) {
    if (gate && *gate != 1u) return;
    float m = 0.f;
    for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < n_rows * F; i += (int64_t)gridDim.x * 1024) {
        const int c = (int)(i % F);
        float4 a = *reinterpret_cast<const float4*>(hs + i);
        const float4 g = *reinterpret_cast<const float4*>(hs + n_rows * F + i);
        const float4 r = *reinterpret_cast<const float4*>(r_mag + c);
        a.x = a.x * expf(r.x) + g.x; a.y = a.y * expf(r.y) + g.y; a.z = a.z * expf(r.z) + g.z; a.w = a.w * expf(r.w) + g.w;
        m = fmaxf(fmaxf(m, fmaxf(fabsf(a.x), fabsf(a.y))), fmaxf(fabsf(a.z), fabsf(a.w)));
        *reinterpret_cast<float4*>(hs + i) = a;
    }
    if (amax) {
        m = wave_max(m);
        if ((threadIdx.x & 63) == 0) atomicMax(amax + ((blockIdx.x * 4 + (threadIdx.x >> 6)) & (DG_AMAX_SLOTS - 1)), __float_as_uint(m));
    }
}

// per feature: gr_mag = sum_n dM (mag_pre - b_mag) = sum_n dM f - b_mag gb_mag (dM != 0 only where f = mag_pre > 0);
// colsum(dP) = e^r gb_mag + gb_gate -> dpsum (the encoder-input term of gb_dec)
__global__ __launch_bounds__(256) void gated_vec_kernel(const float* __restrict__ sdmf, const float* __restrict__ gb_mag,
                                                        const float* __restrict__ gb_gate, const float* __restrict__ b_mag,
                                                        const float* __restrict__ r_mag, float* __restrict__ gr_mag,
                                                        float* __restrict__ dpsum, int F, const uint32_t* __restrict__ gate) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (gate && *gate != 1u) return;
    if (j >= F) return;
    gr_mag[j] = sdmf[j] - b_mag[j] * gb_mag[j];
    dpsum[j] = expf(r_mag[j]) * gb_mag[j] + gb_gate[j];
}

// gW_dec[j] += coef * pgsum[j] * W_dec[j] / ||W_dec[j]||: the decoder-norm factor of the L1 term (sae.py:780-784); one wave per row
__global__ __launch_bounds__(256) void gated_l1_rows_kernel(float* __restrict__ gW_dec, const float* __restrict__ W_dec,
                                                            const float* __restrict__ pgsum, float coef, int F, int d) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= F) return;
    if (pgsum[j] == 0.f) return;                               // (no token opened this gate: a zero term; most rows of a sparse step)
    // (rows of up to 64 * L1_NE elements: the row of W_dec and of gW_dec in registers, all loads in flight -- two loops of one dependent
    // load per trip were 24 round trips to memory per row; same lane mapping, same order)
    constexpr int L1_NE = 20;
    if (d <= 64 * L1_NE) {
        float wv[L1_NE], gv[L1_NE];
#pragma unroll
        for (int u = 0; u < L1_NE; ++u) {
            const int c = lane + 64 * u;
            wv[u] = c < d ? W_dec[(int64_t)j * d + c] : 0.f;
            gv[u] = c < d ? gW_dec[(int64_t)j * d + c] : 0.f;
        }
        float sq = 0.f;
#pragma unroll
        for (int u = 0; u < L1_NE; ++u)
            if (lane + 64 * u < d) sq += wv[u] * wv[u];
        sq = wave_sum(sq);
        const float s = coef * pgsum[j] / sqrtf(sq);
#pragma unroll
        for (int u = 0; u < L1_NE; ++u) {
            const int c = lane + 64 * u;
            if (c < d) gW_dec[(int64_t)j * d + c] = gv[u] + s * wv[u];
        }
        return;
    }
    float sq = 0.f;
    for (int c = lane; c < d; c += 64) { const float w = W_dec[(int64_t)j * d + c]; sq += w * w; }
    sq = wave_sum(sq);
    const float s = coef * pgsum[j] / sqrtf(sq);
    for (int c = lane; c < d; c += 64) gW_dec[(int64_t)j * d + c] += s * W_dec[(int64_t)j * d + c];
}

__global__ __launch_bounds__(256) void gated_axpy_kernel(float* __restrict__ y, const float* __restrict__ x, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] += x[i];
}
}  // namespace

int sae_gated_gbdec(const pv_sae_desc& d, const pv_sae_state* st, const float* dYs, int N, float* tmpd, float* cspart, unsigned char* wsb,
                    const SaeWs& ws, hipStream_t stream) {
    const int D = d.d_in;
    int rc = sae_gbdec(d, st, dYs, N, wsb, ws, stream, SAE_DY_TO_GB_DEC);                  // colsum(dY) - W_enc gb_enc (= colsum(dP) for now)
    if (rc) return rc;
    rc = sae_colsum(dYs + (size_t)N * D, N, D, tmpd, 2.0f, cspart, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(gated_axpy_kernel, dim3((D + 255) / 256), dim3(256), 0, stream, st->gb_dec, (const float*)tmpd, D);
    PV_LAUNCH_CHECK("gated_axpy_kernel");
    PV_HIP_CHECK(hipMemsetAsync(st->gb_enc, 0, (size_t)d.d_sae * 4, stream));      // b_enc takes no part in a gated SAE
    return PV_OK;
}

// ------------------------------------------------------------------------------------------------
// The gated step in sparse form (pv_sae_gated_step_sparse; the dense form and the mathematics: above).
// A gated SAE's forward is sparse in the OPEN GATES: feature_acts, relu(gate_pre) and every gradient behind them vanish where
// gate_pre <= 0 (sae.py:703-716, :773-792).  The selection (relu_select_kernel<GATED>) leaves, per token, the list of its open gates
// with both values per pair {f = feature_acts, g = relu(gate_pre)}; from there the step is the k-sparse machinery with TWO decoder
// terms per pair:
//     decode (ONE gather of W_dec[j] per pair):  reconstruction = sum f W_dec[j] (+ LN-out, mse, dY, dM = (dY . W_dec[j]) [f > 0]),
//                                                via the gate   = sum g W_dec[j] (aux loss against sae_in, dVia, dG = dVia . W_dec[j] + l1 / N)
//     backward (bwd_walk<DUAL>):  gW_dec[j] = sum f dY[n] + g dVia[n],  gW_enc^T[j] = sum dP sae_in[n],  gb_enc[j] = sum dP = colsum(dP)
//     with dP = dM e^r + dG (parked in gb_enc for gb_dec, as the dense form does)
// ------------------------------------------------------------------------------------------------
namespace {
template <int V4>
__global__ __launch_bounds__(256) void gated_decode_kernel(
    const float* __restrict__ x, const float* __restrict__ sae_in, const float* __restrict__ W_dec, const float* __restrict__ b_dec,
    const int32_t* __restrict__ idx, const float* __restrict__ valf, const float* __restrict__ valg, const float* __restrict__ mu,
    const float* __restrict__ sd, const float* __restrict__ norm, float* __restrict__ sae_out, float* __restrict__ dY,
    float* __restrict__ dVia, float* __restrict__ dM, float* __restrict__ dG, float* __restrict__ mse_part, float* __restrict__ aux_part,
    int n_tok, int d, int k, float grad_scale /* 2 / (N d_in) */, float aux_scale /* 2 / N */, float dh_add /* l1 / N */,
    const uint32_t* __restrict__ tok_cnt, const uint32_t* __restrict__ gate) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= n_tok) return;
    if (*gate != 0u) return;
    bool ok[V4];
    int col[V4];
#pragma unroll
    for (int i = 0; i < V4; ++i) {
        col[i] = 4 * lane + 256 * i;
        ok[i] = col[i] < d;
    }
    float4 af[V4], ag[V4];
#pragma unroll
    for (int i = 0; i < V4; ++i) { af[i] = make_float4(0.f, 0.f, 0.f, 0.f); ag[i] = af[i]; }
    const int32_t* ir = idx + (int64_t)n * k;
    const float* fr = valf + (int64_t)n * k;
    const float* gr = valg + (int64_t)n * k;
    const int k_walk = min(k, (int)((tok_cnt[n] + 3u) & ~3u));       // (slots beyond it are holes: g = 0)
    for (int s = 0; s < k_walk; s += 4) {
        float a[4], b[4];
        float4 w[4][V4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int ju = ir[s + u];
            a[u] = fr[s + u];
            b[u] = gr[s + u];
            const float* wr = W_dec + (int64_t)ju * d;
#pragma unroll
            for (int i = 0; i < V4; ++i) w[u][i] = ld4(wr + col[i], ok[i] && b[u] != 0.f);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)                       // (slot order: fixed)
#pragma unroll
            for (int i = 0; i < V4; ++i) {
                af[i].x += a[u] * w[u][i].x; af[i].y += a[u] * w[u][i].y; af[i].z += a[u] * w[u][i].z; af[i].w += a[u] * w[u][i].w;
                ag[i].x += b[u] * w[u][i].x; ag[i].y += b[u] * w[u][i].y; ag[i].z += b[u] * w[u][i].z; ag[i].w += b[u] * w[u][i].w;
            }
    }
    const float m = mu[n], sdv = sd[n], nf = norm[n];
    float lf = 0.f, lg = 0.f;
    float4 gf[V4], gg[V4];
#pragma unroll
    for (int i = 0; i < V4; ++i) {
        gf[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        gg[i] = gf[i];
        if (ok[i]) {
            const float4 bd = *reinterpret_cast<const float4*>(b_dec + col[i]);
            const float4 xv = *reinterpret_cast<const float4*>(x + (int64_t)n * d + col[i]);
            const float4 sv = *reinterpret_cast<const float4*>(sae_in + (int64_t)n * d + col[i]);
            float4 o, e;
            o.x = (af[i].x + bd.x) * sdv + m; o.y = (af[i].y + bd.y) * sdv + m;          // as sae_decode_kernel / gated_finish_kernel
            o.z = (af[i].z + bd.z) * sdv + m; o.w = (af[i].w + bd.w) * sdv + m;
            e.x = o.x - xv.x; e.y = o.y - xv.y; e.z = o.z - xv.z; e.w = o.w - xv.w;
            if (sae_out) *reinterpret_cast<float4*>(sae_out + (int64_t)n * d + col[i]) = o;
            lf += (e.x * e.x) / nf + (e.y * e.y) / nf + (e.z * e.z) / nf + (e.w * e.w) / nf;
            gf[i].x = grad_scale * e.x / nf * sdv; gf[i].y = grad_scale * e.y / nf * sdv;
            gf[i].z = grad_scale * e.z / nf * sdv; gf[i].w = grad_scale * e.w / nf * sdv;
            *reinterpret_cast<float4*>(dY + (int64_t)n * d + col[i]) = gf[i];
            e.x = ag[i].x + bd.x - sv.x; e.y = ag[i].y + bd.y - sv.y; e.z = ag[i].z + bd.z - sv.z; e.w = ag[i].w + bd.w - sv.w;
            lg += e.x * e.x + e.y * e.y + e.z * e.z + e.w * e.w;                          // sae.py:786-792
            gg[i].x = aux_scale * e.x; gg[i].y = aux_scale * e.y; gg[i].z = aux_scale * e.z; gg[i].w = aux_scale * e.w;
            *reinterpret_cast<float4*>(dVia + (int64_t)n * d + col[i]) = gg[i];
        }
    }
    lf = wave_sum(lf);
    lg = wave_sum(lg);
    if (lane == 0) { mse_part[n] = lf; aux_part[n] = lg; }
    for (int s = 0; s < k_walk; s += 4) {
        float df[4], dg[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int ju = ir[s + u];
            const bool live = gr[s + u] > 0.f;                    // (wave-uniform)
            const float* wr = W_dec + (int64_t)ju * d;
            float tf = 0.f, tg = 0.f;
#pragma unroll
            for (int i = 0; i < V4; ++i) {
                const float4 wv = ld4(wr + col[i], ok[i] && live);
                tf += dot4(gf[i], wv);
                tg += dot4(gg[i], wv);
            }
            df[u] = tf;
            dg[u] = tg;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                df[u] += __shfl_xor(df[u], o, 64);
                dg[u] += __shfl_xor(dg[u], o, 64);
            }
        if (lane < 4) {
            const float sf = lane == 0 ? df[0] : (lane == 1 ? df[1] : (lane == 2 ? df[2] : df[3]));
            const float sg = lane == 0 ? dg[0] : (lane == 1 ? dg[1] : (lane == 2 ? dg[2] : dg[3]));
            dM[(int64_t)n * k + s + lane] = fr[s + lane] > 0.f ? sf : 0.f;                    // (dY W_dec^T) [f > 0]
            dG[(int64_t)n * k + s + lane] = gr[s + lane] > 0.f ? sg + dh_add : 0.f;           // (dVia W_dec^T + l1 / N) [gate_pre > 0]
        }
    }
}

// dP = dM e^r + dG per pair (sae.py:708-712 backwards); holes (never written by the decode kernel) -> 0
__global__ __launch_bounds__(256) void gated_pairs_kernel(const int32_t* __restrict__ idx, const uint32_t* __restrict__ wpos,
                                                          const float* __restrict__ dM, const float* __restrict__ dG,
                                                          const float* __restrict__ r_mag, float* __restrict__ dP, int n_pairs,
                                                          const uint32_t* __restrict__ gate) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pairs || *gate != 0u) return;
    dP[i] = wpos[i] != 0xffffffffu ? dM[i] * expf(r_mag[idx[i]]) + dG[i] : 0.f;
}

// per feature, over its list (ascending token order): gb_gate = sum dG, gb_mag = sum dM, gr_mag = sum dM (mag_pre - b_mag) = sum dM f -
// b_mag gb_mag, pgsum = sum relu(gate_pre) (the decoder-norm factor of the L1 term), the firing count of feature_acts + the
// statistics (train_sae.py:356-361).  One wave per feature.
__global__ __launch_bounds__(256) void gated_feat_kernel(const uint32_t* __restrict__ offs, const int32_t* __restrict__ pairs,
                                                         const float* __restrict__ valf, const float* __restrict__ valg,
                                                         const float* __restrict__ dM, const float* __restrict__ dG,
                                                         const float* __restrict__ b_mag, int F, float* __restrict__ gb_gate,
                                                         float* __restrict__ gb_mag, float* __restrict__ gr_mag, float* __restrict__ pgsum,
                                                         float* __restrict__ fire_count, float* __restrict__ act_freq,
                                                         float* __restrict__ n_since_fired, int update_stats,
                                                         const uint32_t* __restrict__ gate) {
    if (*gate != 0u) return;
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= F) return;
    const uint32_t beg = offs[j], end = offs[j + 1];
    float sg = 0.f, sm = 0.f, smf = 0.f, sp = 0.f, fired = 0.f;
#pragma unroll 4
    for (uint32_t q = beg + lane; q < end; q += 64) {      // (unrolled: the gathers of four trips in flight; the sums in order)
        const int p = pairs[q];
        const float f = valf[p], m = dM[p];
        sg += dG[p];
        sm += m;
        smf += m * f;
        sp += valg[p];
        fired += f > 0.f ? 1.f : 0.f;
    }
    sg = wave_sum(sg); sm = wave_sum(sm); smf = wave_sum(smf); sp = wave_sum(sp); fired = wave_sum(fired);
    if (lane != 0) return;
    gb_gate[j] = sg;
    gb_mag[j] = sm;
    gr_mag[j] = smf - b_mag[j] * sm;
    pgsum[j] = sp;
    if (fire_count) fire_count[j] = fired;
    if (update_stats) {
        act_freq[j] += fired;
        n_since_fired[j] = fired > 0.f ? 0.f : n_since_fired[j] + 1.f;
    }
}

// scalars: 1 mse, 6 aux, 4 l1, 2 l0, 0 their sum (sae.py:748); fixed summation order
__global__ __launch_bounds__(256) void gated_sparse_scalars_kernel(const float* __restrict__ mse_part, const float* __restrict__ aux_part,
                                                                   const float* __restrict__ l1part, const float* __restrict__ l0part,
                                                                   int n_tok, float s_mse, float s_aux, float s_l1, float s_l0,
                                                                   float* __restrict__ scalars, const uint32_t* __restrict__ gate) {
    if (*gate != 0u) return;
    __shared__ float red[4][4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float a = 0.f, b = 0.f, c = 0.f, e = 0.f;
#pragma unroll 4
    for (int i = threadIdx.x; i < n_tok; i += 256) { a += mse_part[i]; b += aux_part[i]; c += l1part[i]; e += l0part[i]; }
    a = wave_sum(a); b = wave_sum(b); c = wave_sum(c); e = wave_sum(e);
    if (lane == 0) { red[0][wv] = a; red[1][wv] = b; red[2][wv] = c; red[3][wv] = e; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float mse = ((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) * s_mse;
        const float aux = ((red[1][0] + red[1][1]) + (red[1][2] + red[1][3])) * s_aux;
        const float l1 = ((red[2][0] + red[2][1]) + (red[2][2] + red[2][3])) * s_l1;
        scalars[1] = mse; scalars[6] = aux; scalars[4] = l1;
        scalars[2] = ((red[3][0] + red[3][1]) + (red[3][2] + red[3][3])) * s_l0;
        scalars[0] = mse + l1 + aux;
    }
}

struct GatedSparseWs {                        // the workspace of pv_sae_relu_sparse for the gated step: relu_carve's, then the second value per pair
    ReluWs rw;
    size_t total, valg, dM, dG, l0part;
};
GatedSparseWs gated_sparse_carve(const pv_sae_desc& d, int n_tokens, int cap) {
    GatedSparseWs w;
    w.rw = relu_carve(d, n_tokens, cap);
    size_t off = w.rw.total;
    auto take = [&](size_t bytes) { size_t o = off; off += (size_t)pv_align_up((int64_t)bytes, 256); return o; };
    const size_t N = (size_t)n_tokens, P = N * (size_t)cap;
    w.valg = take(P * 4);
    w.dM = take(P * 4);
    w.dG = take(P * 4);
    w.l0part = take(N * 4);
    w.total = off + 256;
    return w;
}

// dYs: [2N, d_in] = [dY; dVia] (the dense form's layout), auxpart: [N], pgsum: [d_sae] -- regions of the gated scratch the two
// forms share, so that everything behind them (the decoder-norm term, gb_dec) runs once.  Leaves colsum(dP) in st->gb_enc.
int sae_gated_sparse(pv_sae_plan* plan, pv_sae_state* st, const float* x, int N, int n_global, int cap, float l1_coefficient,
                     int update_stats, unsigned char* rwb, const GatedSparseWs& gs, pv_sae_out* out, unsigned char* wsb, const SaeWs& ws,
                     float* dYs, float* auxpart, float* pgsum, hipStream_t stream) {
    const pv_sae_desc& d = plan->d;
    const pv_sae_gated& t = st->gt;
    const ReluWs& rw = gs.rw;
    const int D = d.d_in, F = d.d_sae, n_pairs = N * cap;
    const float ng = (float)n_global;
    uint32_t* mode = (uint32_t*)(rwb + rw.mode);
    int32_t* idx = (int32_t*)(rwb + rw.idx);
    float* valf = (float*)(rwb + rw.val);
    float* valg = (float*)(rwb + gs.valg);
    uint32_t* wpos = (uint32_t*)(rwb + rw.wpos);
    uint32_t* tok_cnt = (uint32_t*)(rwb + rw.tok_cnt);
    float* l1part = (float*)(rwb + rw.l1part);
    float* l0part = (float*)(rwb + gs.l0part);
    float* dM = (float*)(rwb + gs.dM);
    float* dG = (float*)(rwb + gs.dG);
    float* dP = (float*)(rwb + rw.dh);
    const float* sae_in = (const float*)(wsb + ws.sae_in);
    float* dVia = dYs + (size_t)N * D;
    int rc;
    {
        ProfScope prof(PV_PROF_SAE_ENC, stream, 2.0 * N * (double)D * F, ((double)N * D + (double)D * F) * 2.0);
        rc = sae_encode_relu(d, st, N, cap, idx, valf, tok_cnt, l1part, (uint32_t*)(rwb + rw.cand_cnt), rwb + rw.cand,
                             (uint32_t*)(wsb + ws.cnt), wpos, mode, (const float*)out->scalars, wsb, ws, stream, l0part, valg);
        if (rc) return rc;
    }
    ProfScope prof(PV_PROF_SAE_BWD, stream, 6.0 * n_pairs * (double)D * 2.0, 0.0);
    const dim3 grid((N + 3) / 4), block(256);
#define CALL(V)                                                                                                                   \
    hipLaunchKernelGGL((gated_decode_kernel<V>), grid, block, 0, stream, x, sae_in, (const float*)st->W_dec, (const float*)st->b_dec, \
                       (const int32_t*)idx, (const float*)valf, (const float*)valg, (const float*)(wsb + ws.mu),                    \
                       (const float*)(wsb + ws.sd), (const float*)(wsb + ws.norm), out->sae_out, dYs, dVia, dM, dG,                 \
                       (float*)(wsb + ws.loss_part), auxpart, N, D, cap, 2.0f / (ng * (float)D), 2.0f / ng, l1_coefficient / ng,   \
                       (const uint32_t*)tok_cnt, (const uint32_t*)mode)
    V4_DISPATCH(D, CALL);
#undef CALL
    PV_LAUNCH_CHECK("gated_decode_kernel");
    hipLaunchKernelGGL(gated_pairs_kernel, dim3((n_pairs + 255) / 256), block, 0, stream, (const int32_t*)idx, (const uint32_t*)wpos,
                       (const float*)dM, (const float*)dG, (const float*)t.r_mag, dP, n_pairs, (const uint32_t*)mode);
    PV_LAUNCH_CHECK("gated_pairs_kernel");
    SaeBwd b;                                                       // (statistics and fire_count: gated_feat_kernel)
    b.N = N; b.k = cap; b.idx = idx; b.val = valf; b.dY = dYs; b.sae_in = sae_in; b.scalars = out->scalars;
    b.tail = relu_tail(rwb, rw);                                    // (tail.dh = dP)
    b.gate = mode; b.val_b = valg; b.dY_b = dVia;
    rc = sae_csr_backward(plan, st, b, wsb, ws, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(gated_feat_kernel, dim3((F + 3) / 4), block, 0, stream, (const uint32_t*)(wsb + ws.offs), (const int32_t*)b.tail.pairs,
                       (const float*)valf, (const float*)valg, (const float*)dM, (const float*)dG, (const float*)t.b_mag, F, t.gb_gate,
                       t.gb_mag, t.gr_mag, pgsum, out->fire_count, st->act_freq_scores, st->n_fwd_since_fired, update_stats,
                       (const uint32_t*)mode);
    hipLaunchKernelGGL(gated_sparse_scalars_kernel, dim3(1), block, 0, stream, (const float*)(wsb + ws.loss_part), (const float*)auxpart,
                       (const float*)l1part, (const float*)l0part, N, 1.0f / (ng * (float)D), 1.0f / ng, l1_coefficient / ng,
                       1.0f / (float)N, out->scalars, (const uint32_t*)mode);
    PV_LAUNCH_CHECK("gated sparse kernels");
    return PV_OK;
}
}  // namespace

extern "C" size_t pv_sae_gated_scratch_bytes(const pv_sae_plan* plan, int32_t n_tokens) {
    if (!plan || n_tokens < 1) return 0;
    return gated_carve(plan->d, n_tokens).total;
}

// sp != NULL (pv_sae_gated_step_sparse): the step runs sparse where the batch allows it, as pv_sae_relu_step does -- the open gates of
// every token as a list of at most sp->cap pairs (sae_gated_sparse); a batch that cannot be held raises the device-side mode
// word and the dense GEMMs below run instead (every kernel of either form leaves at once in the other's mode; same results either way).
static int gated_step_impl(pv_sae_plan* plan, pv_sae_state* st, const float* x, int32_t N, const float* batch_mean, int32_t n_global,
                           int32_t flags, float l1_coefficient, const pv_sae_relu_sparse* sp, pv_sae_out* out, void* workspace,
                           size_t workspace_bytes, void* stream_) {
    const int update_stats = (flags & PV_SAE_UPDATE_STATS) ? 1 : 0;
    PV_REQUIRE(plan && st && x && out && workspace && out->scalars, "null argument");
    PV_REQUIRE(sae_is_gated(st) && !sae_is_tc(st), "pv_sae_gated_step needs a gated state (pv_sae_state.gt) and no transcoder");
    const pv_sae_gated& t = st->gt;
    PV_REQUIRE(t.r_mag && t.b_mag && t.gb_gate && t.gr_mag && t.gb_mag && t.scratch, "gated state");
    PV_REQUIRE(st->W_dec && st->b_dec && st->gW_enc && st->gW_dec && st->gb_enc && st->gb_dec && st->W_encT, "state");
    PV_REQUIRE(!update_stats || (st->act_freq_scores && st->n_fwd_since_fired), "stats buffers");
    PV_REQUIRE(flags & PV_SAE_RENORM_DECODER, "pv_sae_gated_step: PV_SAE_RENORM_DECODER is required (unit decoder rows in the L1 term)");
    const pv_sae_desc& d = plan->d;
    PV_REQUIRE(N >= 1 && N <= d.max_tokens, "n_tokens exceeds plan max_tokens");
    PV_REQUIRE(n_global >= N, "n_global must be >= n_tokens");
    PV_REQUIRE(d.d_in % 8 == 0 && d.d_sae % 8 == 0, "the gated step needs d_in and d_sae to be multiples of 8");
    const SaeWs ws = sae_carve(d);
    PV_REQUIRE(workspace_bytes >= ws.total && ((uintptr_t)workspace & 255) == 0, "workspace too small / misaligned");
    const GatedWs gw = gated_carve(d, N);
    PV_REQUIRE(t.scratch_bytes >= gw.total && ((uintptr_t)t.scratch & 255) == 0, "gated scratch too small / misaligned");
    hipStream_t stream = (hipStream_t)stream_;
    unsigned char* wsb = (unsigned char*)workspace;
    unsigned char* gb = (unsigned char*)t.scratch;
    const bool sparse = sp && pv_sae_relu_sparse_ok(d) && st->W_enc16T && st->enc_colsq;
    GatedSparseWs gs = {};
    unsigned char* rwb = nullptr;
    if (sp) {
        PV_REQUIRE(sp->cap >= 4 && sp->cap <= PV_SAE_RELU_CAP_MAX && sp->cap % 4 == 0, "pv_sae_relu_sparse.cap: a multiple of 4 in [4, 256]");
        gs = gated_sparse_carve(d, N, sp->cap);
        PV_REQUIRE(sp->workspace && sp->workspace_bytes >= gs.total && ((uintptr_t)sp->workspace & 255) == 0,
                   "pv_sae_relu_sparse workspace too small / misaligned (pv_sae_gated_sparse_workspace_bytes)");
        rwb = (unsigned char*)sp->workspace;
    }
    const uint32_t* mode = sp ? (const uint32_t*)(rwb + gs.rw.mode) : nullptr;
    plan->live_offs = nullptr;
    plan->renorm_pending = false;
    const int F = d.d_sae, D = d.d_in;
    int rc = pv_sae_renorm_decoder(plan, st, stream_);                   // train_sae.py:307
    if (rc) return rc;
    rc = sae_prep(d, x, (const float*)st->b_dec, batch_mean, N, sparse, wsb, ws, stream);
    const float ng = (float)n_global;
    if (rc) return rc;
    float* hs = (float*)(gb + gw.hs);
    float* dYs = (float*)(gb + gw.dys);
    float* kpart = (float*)(gb + gw.kpart);
    float* sae_in = (float*)(wsb + ws.sae_in);
    float* colpart = (float*)(wsb + ws.dense_colpart);
    float* colpart2 = (float*)(gb + gw.colpart2);
    float* rowpart = (float*)(wsb + ws.dense_rowpart);
    float* pgsum = (float*)(gb + gw.vec0);
    float* sdmf = (float*)(gb + gw.vec1);
    const int rblk = (N + 63) / 64, cblk = (F + 63) / 64, nb_f = (F + 255) / 256;
    float* blk_tot = (float*)(wsb + ws.sqpart);
    // operand maxima of the split-fp16 GEMMs (see dense_gemm_kernel): sae_in, W_enc^T, hs = [f; relu(gate)], W_dec, dYs = [dY; dVia],
    // dM, dG, dP
    const DenseAmax am = {(uint32_t*)(wsb + ws.dense_amax)};
    enum { AM_X = DG_AM_X, AM_WENC = DG_AM_WENC, AM_HS = 2, AM_WDEC = DG_AM_WDEC, AM_DY = 4, AM_DM = 5, AM_DG = 6, AM_DP = 7 };
    const bool split = dense_split_ok(d, N);
    if (sparse) {
        rc = sae_gated_sparse(plan, st, x, N, n_global, sp->cap, l1_coefficient, update_stats, rwb, gs, out, wsb, ws, dYs,
                              (float*)(gb + gw.auxpart), pgsum, stream);
        if (rc) return rc;
    } else if (mode) {
        sae_set_u32((uint32_t*)(rwb + gs.rw.mode), 1u, stream);
    }
    if (split) {
        rc = dense_absmax3(d, st, sae_in, N, am.base, mode, stream);
        if (rc) return rc;
    }
    {
        ProfScope prof(PV_PROF_SAE_ENC, stream, 2.0 * N * (double)D * F, ((double)N * D + (double)D * F + 2.0 * N * F) * 4.0);
        // G1: p = sae_in @ W_enc once; both paths in the epilogue
        DenseGemm g = {};
        g.A = sae_in; g.lda = D; g.B = st->W_encT; g.ldb = D; g.M = N; g.N = F; g.K = D; g.k_chunk = D;
        g.out = hs; g.ldo = F; g.out2 = hs + (size_t)N * F; g.bias = t.b_gate; g.bias2 = t.b_mag; g.cscale = t.r_mag;
        g.colpart = colpart; g.colpart2 = colpart2; g.rowpart = rowpart; g.gate = mode;
        if (split) { g.a_max = am(AM_X); g.b_max = am(AM_WENC); g.amax_out = am(AM_HS); }
        rc = launch_dense_gemm<false, false, DG_EPI_GENC>(g, 1, stream);
        if (rc) return rc;
        rc = dense_colreduce(colpart, rblk, F, out->fire_count ? out->fire_count : (float*)(wsb + ws.rowsq), st->act_freq_scores,
                             st->n_fwd_since_fired, update_stats, blk_tot, mode, stream);
        if (rc) return rc;
        rc = dense_colreduce(colpart2, rblk, F, pgsum, mode, stream);
        if (rc) return rc;
        sae_reduce_sum(blk_tot, out->scalars, nb_f, 1.0f / (float)N, 2, -1, stream, mode, 1u);                        // l0
        sae_reduce_sum(rowpart, out->scalars, rblk * cblk, l1_coefficient / ng, 4, -1, stream, mode, 1u);             // l1 (unit decoder rows)
    }
    {
        ProfScope prof(PV_PROF_SAE_BWD, stream, 14.0 * N * (double)D * F, 0.0);
        // G2: [f; relu(gate)] @ W_dec, split over K
        const int S = PV_SAE_DENSE_SPLITK;
        DenseGemm g = {};
        g.A = hs; g.lda = F; g.B = st->W_dec; g.ldb = D; g.M = 2 * N; g.N = D; g.K = F;
        g.k_chunk = ((F + S - 1) / S + DG_KSLAB - 1) / DG_KSLAB * DG_KSLAB;
        g.out = kpart; g.ldo = D; g.out_zstride = (int64_t)2 * N * D; g.gate = mode;
        if (split) { g.a_max = am(AM_HS); g.b_max = am(AM_WDEC); }
        rc = launch_dense_gemm<false, true, DG_EPI_STORE>(g, S, stream);
        if (rc) return rc;
        hipLaunchKernelGGL(gated_finish_kernel, dim3((2 * N + 3) / 4), dim3(256), 0, stream, x, (const float*)sae_in, (const float*)kpart, S,
                           (int64_t)2 * N * D, (const float*)st->b_dec, (const float*)(wsb + ws.mu), (const float*)(wsb + ws.sd),
                           (const float*)(wsb + ws.norm), out->sae_out, dYs, (float*)(wsb + ws.loss_part), (float*)(gb + gw.auxpart), N, D,
                           2.0f / (ng * (float)D), 2.0f / ng, mode, split ? am(AM_DY) : (uint32_t*)nullptr);
        PV_LAUNCH_CHECK("gated_finish_kernel");
        sae_reduce_sum((const float*)(wsb + ws.loss_part), out->scalars, N, 1.0f / (ng * (float)D), 1, -1, stream, mode, 1u);
        sae_reduce_sum((const float*)(gb + gw.auxpart), out->scalars, N, 1.0f / ng, 6, -1, stream, mode, 1u);
        hipLaunchKernelGGL(gated_loss_kernel, dim3(1), dim3(1), 0, stream, out->scalars, mode);
        // G4: gW_dec = [f; relu(gate)]^T @ [dY; dVia] (K = 2N); the decoder-norm factor of the L1 term is added behind both forms
        DenseGemm g4 = {};
        g4.A = hs; g4.lda = F; g4.B = dYs; g4.ldb = D; g4.M = F; g4.N = D; g4.K = 2 * N; g4.k_chunk = 2 * N;
        g4.out = st->gW_dec; g4.ldo = D; g4.gate = mode;
        if (split) { g4.a_max = am(AM_HS); g4.b_max = am(AM_DY); }
        rc = launch_dense_gemm<true, true, DG_EPI_STORE>(g4, 1, stream);
        if (rc) return rc;
        // G3a: dM = (dY @ W_dec^T) [f > 0] over f; column sums = gb_mag, of dM * f = the raw term of gr_mag
        DenseGemm g3 = {};
        g3.A = dYs; g3.lda = D; g3.B = st->W_dec; g3.ldb = D; g3.M = N; g3.N = F; g3.K = D; g3.k_chunk = D;
        g3.out = hs; g3.ldo = F; g3.colpart = colpart; g3.colpart2 = colpart2; g3.add = 0.f; g3.gate = mode;
        if (split) { g3.a_max = am(AM_DY); g3.b_max = am(AM_WDEC); g3.amax_out = am(AM_DM); }
        rc = launch_dense_gemm<false, false, DG_EPI_DH>(g3, 1, stream);
        if (rc) return rc;
        rc = dense_colreduce(colpart, rblk, F, t.gb_mag, mode, stream);
        if (rc) return rc;
        rc = dense_colreduce(colpart2, rblk, F, sdmf, mode, stream);
        if (rc) return rc;
        // G3b: dG = (dVia @ W_dec^T + l1 / N) [gate > 0] over relu(gate); column sums = gb_gate
        g3.A = dYs + (size_t)N * D; g3.out = hs + (size_t)N * F; g3.colpart2 = nullptr; g3.add = l1_coefficient / ng;
        if (split) g3.amax_out = am(AM_DG);
        rc = launch_dense_gemm<false, false, DG_EPI_DH>(g3, 1, stream);
        if (rc) return rc;
        rc = dense_colreduce(colpart, rblk, F, t.gb_gate, mode, stream);
        if (rc) return rc;
        // gr_mag; colsum(dP) parked in gb_enc for the bias-gradient kernels below
        hipLaunchKernelGGL(gated_vec_kernel, dim3(nb_f), dim3(256), 0, stream, (const float*)sdmf, (const float*)t.gb_mag,
                           (const float*)t.gb_gate, (const float*)t.b_mag, (const float*)t.r_mag, t.gr_mag, st->gb_enc, F, mode);
        // dP = dM e^r + dG, then G5: gW_enc^T = dP^T @ sae_in
        // (a bounded grid walking the rows: in the sparse form's mode the launch is empty, and ~100k empty workgroups are 20 us)
        hipLaunchKernelGGL(gated_dp_kernel, dim3((unsigned)std::min<int64_t>(((int64_t)N * F / 4 + 255) / 256, 8192)), dim3(256), 0, stream, hs,
                           (const float*)t.r_mag, (int64_t)N, F, mode, split ? am(AM_DP) : (uint32_t*)nullptr);
        PV_LAUNCH_CHECK("gated elementwise kernels");
        DenseGemm g5 = {};
        g5.A = hs; g5.lda = F; g5.B = sae_in; g5.ldb = D; g5.M = F; g5.N = D; g5.K = N; g5.k_chunk = N;
        g5.out = st->gW_enc; g5.ldo = D; g5.gate = mode;
        if (split) { g5.a_max = am(AM_DP); g5.b_max = am(AM_X); }
        rc = launch_dense_gemm<true, true, DG_EPI_STORE>(g5, 1, stream);
        if (rc) return rc;
    }
    // behind either form: dYs = [dY; dVia], pgsum = colsum(relu(gate_pre)), colsum(dP) in gb_enc, gW_dec without the L1 term
    hipLaunchKernelGGL(gated_l1_rows_kernel, dim3((F + 3) / 4), dim3(256), 0, stream, st->gW_dec, (const float*)st->W_dec,
                       (const float*)pgsum, l1_coefficient / ng, F, D);
    // gb_dec = colsum(dY) + 2 colsum(dVia) - W_enc colsum(dP): b_dec sits in the decoder twice and in sae_in, which is also
    // the auxiliary loss's target
    return sae_gated_gbdec(d, st, dYs, N, (float*)(gb + gw.tmpd), (float*)(gb + gw.cspart), wsb, ws, stream);
}

extern "C" int pv_sae_gated_step(pv_sae_plan* plan, pv_sae_state* st, const float* x, int32_t N, const float* batch_mean, int32_t n_global,
                                 int32_t flags, float l1_coefficient, pv_sae_out* out, void* workspace, size_t workspace_bytes,
                                 void* stream_) {
    return gated_step_impl(plan, st, x, N, batch_mean, n_global, flags, l1_coefficient, nullptr, out, workspace, workspace_bytes, stream_);
}

extern "C" size_t pv_sae_gated_sparse_workspace_bytes(const pv_sae_plan* plan, int32_t n_tokens, int32_t cap) {
    if (!plan || n_tokens < 1 || cap < 4 || cap > PV_SAE_RELU_CAP_MAX || cap % 4) return 0;
    return gated_sparse_carve(plan->d, n_tokens, cap).total;
}

extern "C" int pv_sae_gated_step_sparse(pv_sae_plan* plan, pv_sae_state* st, const float* x, int32_t N, const float* batch_mean,
                                        int32_t n_global, int32_t flags, float l1_coefficient, const pv_sae_relu_sparse* sp,
                                        pv_sae_out* out, void* workspace, size_t workspace_bytes, void* stream_) {
    PV_REQUIRE(sp, "pv_sae_gated_step_sparse: pv_sae_relu_sparse is required (pv_sae_gated_step is the dense form)");
    return gated_step_impl(plan, st, x, N, batch_mean, n_global, flags, l1_coefficient, sp, out, workspace, workspace_bytes, stream_);
}
