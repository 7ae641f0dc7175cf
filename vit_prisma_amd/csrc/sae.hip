// SAE training step for gfx950 (C ABI: pv_sae_* in include/pv_native.h).
//
// Reference semantics: StandardSparseAutoencoder.forward (/root/reference/src/vit_prisma/sae/sae.py:
// 557-645), TopK (:795-810), _compute_mse_loss (:144-149), run-time LayerNorm of the input (:78-93),
// and VisionSAETrainer.train_step (sae/train_sae.py:278-411).  fp32 throughout (the reference's SAE
// config has no bf16, sae/config.py:14-45).
//
// Data flow of one step on N tokens (k-sparse everywhere after the encoder):
//   prep        x -> mu, std (unbiased), x_hat = (x - mu)/(std + eps), sae_in = x_hat - b_dec,
//               norm_n = ||x_n - mean_batch(x)||_2                                    (one wave / token)
//   encode      hidden_pre = sae_in @ W_enc + b_enc      fp32 MFMA GEMM, W_enc read in its own [K][N] layout
//   topk        exact per-row radix select of the k largest -> (idx, relu(val))       (one workgroup / token)
//   decode      sae_out = (sum_s val_s W_dec[idx_s] + b_dec) * std + mu ; err ; loss partials ;
//               dY = 2 err std / (norm N_glob d_in) ; dh_s = dY . W_dec[idx_s]        (one wave / token)
//   csr         active (token, slot) pairs grouped by feature: count -> scan -> fill                       (sae_bwd.hip)
//   backward    per feature j: gW_dec[j,:] = sum a dY[n,:] ; gW_encT[j,:] = sum g sae_in[n,:] ; gb_enc[j] = sum g   (sae_bwd.hip)
//               (rows of both gradients are written coalesced; W_enc's gradient is kept TRANSPOSED,
//               [d_sae][d_in], and transposed back tile-wise inside the Adam kernel)
//   bias grads  gb_dec = colsum(dY) - W_enc @ gb_enc   (the encoder-input path of b_dec, folded into a GEMV)
//   apply       clip coefficient -> remove component parallel to decoder rows -> Adam, fused per tensor            (sae_apply.hip)
// Here: the pre-pass, the exact top-k, the decode kernel (sae_decode), column sums and reductions, the bias gradients (sae_gbdec), the
// plan and its workspace, the transcoder helpers, pv_sae_encode_topk, pv_sae_forward, sae_sparse_tail and pv_sae_step.  The step cut at
// the reconstruction for feature-parallel training: sae_tp.hip; the top-k form of the gated SAE: sae_gated_topk.hip.
#include <math.h>
#include <string.h>

#include "sae_bwd.hpp"
#include "sae_enc.hpp"

namespace {

// ------------------------------------------------------------------------------------------------
// generic helpers
// ------------------------------------------------------------------------------------------------
// column sums of a [rows][d] fp32 matrix (deterministic two-stage reduction).  stage 1: colsum_partial_body (sae_bwd.hpp: also a role
// of csr_post_fill_kernel)
__global__ __launch_bounds__(256) void colsum_partial_kernel(const float* __restrict__ x, float* __restrict__ partial,
                                                             int rows, int d) {
    colsum_partial_body(blockIdx.x, x, partial, rows, d);
}
// stage 2: out[c] = scale * sum_blk partial[blk][c]; 64 columns per workgroup, 16 partial streams per column (the
// 256 partial rows of a 4096-token batch are 16 loads per thread instead of a 64-deep serial chain)
// (returns out[c] on the threads that wrote one -- part 0, c < d -- and 0 elsewhere)
__device__ __forceinline__ float colsum_final_body(int bid, const float* __restrict__ partial, float* __restrict__ out,
                                                   int nblk, int d, float scale) {
    __shared__ float red[16][64];
    const int lane = threadIdx.x & 63, part = threadIdx.x >> 6;
    const int c = bid * 64 + lane;
    float s = 0.f;
    if (c < d) {
#pragma unroll 8
        for (int b = part; b < nblk; b += 16) s += partial[(int64_t)b * d + c];      // (unrolled: the loads of 8 trips in flight, the sum in order)
    }
    red[part][lane] = s;
    __syncthreads();
    if (part == 0 && c < d) {
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) t += red[q][lane];        // fixed order
        out[c] = t * scale;
        return t * scale;
    }
    return 0.f;
}
__global__ __launch_bounds__(1024) void colsum_final_kernel(const float* __restrict__ partial, float* __restrict__ out,
                                                            int nblk, int d, float scale) {
    (void)colsum_final_body(blockIdx.x, partial, out, nblk, d, scale);
}

// ------------------------------------------------------------------------------------------------
// prep: LN-in (sae.py:78-87), sae_in (sae.py:563-565), loss normaliser (sae.py:145-147)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void sae_prep_body(int bid, const float* __restrict__ x, const float* __restrict__ b_dec,
                                              const float* __restrict__ batch_mean, float* __restrict__ sae_in,
                                              _Float16* __restrict__ x16, float* __restrict__ xnorm_out,
                                              float* __restrict__ mu_out, float* __restrict__ std_out,
                                              float* __restrict__ norm_out, int n_tok, int d, int use_ln, float eps,
                                              int d_true) {
    // d_true < d (a transcoder whose input is narrower than its output, pv_sae_transcoder.d_in_true: rows are padded to the common
    // width d): the statistics run over the d_true real columns, the padding of sae_in / x16 is written as exact zeros
    const int lane = threadIdx.x & 63;
    const int n = bid * 4 + (threadIdx.x >> 6);
    if (n >= n_tok) return;
    const float* xr = x + (int64_t)n * d;
    // Rows of up to 64 * PREP_NE elements live in registers: ONE round trip to memory for the row (all of a lane's loads in flight),
    // the three passes below run out of registers.  The loops further down re-read the row from memory with one dependent load per
    // trip -- 3 x 12 round trips at d = 768, 14 of this kernel's 17 us by its waves' PMC lifetimes; they remain for wider rows.  Same
    // operations in the same order either way.
    constexpr int PREP_NE = 20;
    if (d <= 64 * PREP_NE) {
        float xv[PREP_NE], bm[PREP_NE], bd[PREP_NE];
#pragma unroll
        for (int u = 0; u < PREP_NE; ++u) {
            const int i = lane + 64 * u;
            xv[u] = i < d ? xr[i] : 0.f;
            bm[u] = (batch_mean && i < d_true) ? batch_mean[i] : 0.f;
            bd[u] = i < d_true ? b_dec[i] : 0.f;
        }
        float s = 0.f, cn = 0.f;
#pragma unroll
        for (int u = 0; u < PREP_NE; ++u) {
            if (lane + 64 * u < d_true) {
                s += xv[u];
                if (batch_mean) {
                    const float c = xv[u] - bm[u];
                    cn += c * c;
                }
            }
        }
        const float mu = use_ln == 1 ? wave_sum(s) / (float)d_true : 0.f;
        cn = wave_sum(cn);
        float sq = 0.f;
#pragma unroll
        for (int u = 0; u < PREP_NE; ++u) {
            if (lane + 64 * u < d_true) {
                const float c = xv[u] - mu;
                sq += c * c;
            }
        }
        sq = wave_sum(sq);
        const float coeff = use_ln == 2 ? sqrtf((float)d_true) / sqrtf(sq) : 1.f;
        const float sd = use_ln == 1 ? sqrtf(sq / (float)(d_true - 1)) : (use_ln == 2 ? 1.f / coeff : 1.f);
        float s2 = 0.f, amax = 0.f;
#pragma unroll
        for (int u = 0; u < PREP_NE; ++u) {
            const int i = lane + 64 * u;
            if (i < d) {
                const float xh = use_ln == 1 ? (xv[u] - mu) / (sd + eps) : (use_ln == 2 ? xv[u] * coeff : xv[u]);
                const float si = i < d_true ? xh - bd[u] : 0.f;
                sae_in[(int64_t)n * d + i] = si;
                if (x16) x16[(int64_t)n * d + i] = (_Float16)si;
                s2 += si * si;
                amax = fmaxf(amax, fabsf(si));
            }
        }
        s2 = wave_sum(s2);
        amax = wave_max(amax);
        if (lane == 0) {
            mu_out[n] = mu;
            std_out[n] = sd;
            if (batch_mean) norm_out[n] = sqrtf(cn);
            if (xnorm_out) xnorm_out[n] = (amax <= 6.0e4f) ? sqrtf(s2) : INFINITY;
        }
        return;
    }
    // batch_mean == NULL: the loss normaliser is left to a later kernel (the select kernel of the fused pre-pass, SaePre)
    float s = 0.f, cn = 0.f;
    if (batch_mean) {
        for (int i = lane; i < d_true; i += 64) {
            const float v = xr[i];
            s += v;
            const float c = v - batch_mean[i];
            cn += c * c;
        }
    } else {
        for (int i = lane; i < d_true; i += 64) s += xr[i];
    }
    // use_ln: 0 none, 1 "layer_norm" (sae.py:74-90), 2 "constant_norm_rescale" (sae.py:60-72: x * c on the way in with
    // c = sqrt(d_in) / ||x||, / c on the way out -- the step's other kernels only know "out = pre * sd + mu": mu = 0, sd = 1 / c)
    const float mu = use_ln == 1 ? wave_sum(s) / (float)d_true : 0.f;
    cn = wave_sum(cn);
    float sq = 0.f;
    for (int i = lane; i < d_true; i += 64) {
        const float c = xr[i] - mu;
        sq += c * c;
    }
    sq = wave_sum(sq);
    // torch.std: unbiased (divide by d - 1)
    const float coeff = use_ln == 2 ? sqrtf((float)d_true) / sqrtf(sq) : 1.f;
    const float sd = use_ln == 1 ? sqrtf(sq / (float)(d_true - 1)) : (use_ln == 2 ? 1.f / coeff : 1.f);
    float s2 = 0.f, amax = 0.f;
    for (int i = lane; i < d; i += 64) {
        const float xh = use_ln == 1 ? (xr[i] - mu) / (sd + eps) : (use_ln == 2 ? xr[i] * coeff : xr[i]);
        const float si = i < d_true ? xh - b_dec[i] : 0.f;
        sae_in[(int64_t)n * d + i] = si;
        if (x16) x16[(int64_t)n * d + i] = (_Float16)si;       // operand of the filter GEMM (sae_enc_gemm.hip)
        s2 += si * si;
        amax = fmaxf(amax, fabsf(si));
    }
    s2 = wave_sum(s2);
    amax = wave_max(amax);
    if (lane == 0) {
        mu_out[n] = mu;
        std_out[n] = sd;
        if (batch_mean) norm_out[n] = sqrtf(cn);
        // ||sae_in||_2 for the filter's error bound; a row outside the fp16 range (or NaN) is sent to the exact path
        if (xnorm_out) xnorm_out[n] = (amax <= 6.0e4f) ? sqrtf(s2) : INFINITY;
    }
}
__global__ __launch_bounds__(256) void sae_prep_kernel(const float* __restrict__ x, const float* __restrict__ b_dec,
                                                       const float* __restrict__ batch_mean, float* __restrict__ sae_in,
                                                       _Float16* __restrict__ x16, float* __restrict__ xnorm_out,
                                                       float* __restrict__ mu_out, float* __restrict__ std_out,
                                                       float* __restrict__ norm_out, int n_tok, int d, int use_ln, float eps,
                                                       int d_true) {
    sae_prep_body(blockIdx.x, x, b_dec, batch_mean, sae_in, x16, xnorm_out, mu_out, std_out, norm_out, n_tok, d, use_ln, eps, d_true);
}
// The first launch of the fused pre-pass (SaePre): workgroup 0 = the weight bound (below), [1, 1 + nblk) = the 16-row partial column
// sums of x (the batch mean's first stage; nblk = 0 when the caller supplied the mean), the other nb_prep = prep without the loss
// normaliser.  The
// weight bound max_j ||W_enc[:, j]||^2 of the filter's error band + the zeroing of the per-feature pair counters and the fallback
// count (enc_wmax_body, sae_enc.hpp: what sae_wmax_kernel of sae_enc.hip runs where there is no fused pre-pass)
__global__ __launch_bounds__(256) void sae_prep_roles_kernel(const float* __restrict__ x, const float* __restrict__ b_dec,
                                                             float* __restrict__ sae_in, _Float16* __restrict__ x16,
                                                             float* __restrict__ xnorm_out, float* __restrict__ mu_out,
                                                             float* __restrict__ std_out, int n_tok, int d, int use_ln, float eps,
                                                             int d_true, int nb_prep, float* __restrict__ colpart, int nblk,
                                                             const float* __restrict__ colsq, int d_sae, float* __restrict__ wmax_out,
                                                             uint32_t* __restrict__ fb_count, uint32_t* __restrict__ feat_cnt) {
    // (the one workgroup of the weight bound is the launch's longest job: it goes FIRST, the column sums next, the tokens last)
    const int b = blockIdx.x;
    if (b > nblk) {
        sae_prep_body(b - 1 - nblk, x, b_dec, nullptr, sae_in, x16, xnorm_out, mu_out, std_out, nullptr, n_tok, d, use_ln, eps, d_true);
    } else if (b > 0) {
        colsum_partial_body(b - 1, x, colpart, n_tok, d);
    } else {
        enc_wmax_body(colsq, d_sae, wmax_out, fb_count, feat_cnt);
    }
}

// ------------------------------------------------------------------------------------------------
// exact top-k per row by radix select on the order-preserving uint image of the floats
// (TopK.forward, sae.py:795-810: torch.topk -> relu -> scatter; only the selected SET matters)
// ------------------------------------------------------------------------------------------------
constexpr int TOPK_CAP = PV_TOPK_CAP;   // candidate list capacity of the fast path

// Per-row exact top-k, streaming (no per-thread value cache -> ~40 VGPRs, full occupancy):
//   pass 1  each thread streams its share of the row keeping only its maximum
//   T0      the k-th largest of the 256 per-thread maxima is a lower bound of the global k-th largest
//           value (every maximum is an element), found by an all-pairs rank over 256 LDS values
//   pass 2  the row is streamed again (it is L2-resident: 96 KB just read) and the few elements >= T0
//           are compacted into LDS
//   rank    exact rank of every candidate by (value desc, column asc): rank < k -> output slot = rank, so
//           the result is sorted by value like torch.topk and run-to-run deterministic
// Fallback (more than TOPK_CAP candidates: massive ties at the top, e.g. constant rows): MSB-first radix
// select that re-streams the row once per digit.
// `row_list` != nullptr: the workgroups walk rows row_list[blockIdx.x], row_list[blockIdx.x + gridDim.x], ... (the tokens
// the filtered encoder of sae_enc.hip could not decide); otherwise row = blockIdx.x.
// `feat_cnt` / `wpos` (both or neither): every kept (token, slot) with a positive value draws its position inside its
// feature's pair list from feat_cnt[feature] (zeroed by the caller) -- the CSR-by-feature of the backward then needs only
// a scan and an atomic-free scatter.
__device__ void sae_topk_row(const float* __restrict__ hidden, int32_t* __restrict__ idx_out, float* __restrict__ val_out,
                             int d_sae, int k, int64_t row, uint32_t* __restrict__ feat_cnt, uint32_t* __restrict__ wpos);

__global__ __launch_bounds__(256) void sae_topk_kernel(const float* __restrict__ hidden, int32_t* __restrict__ idx_out,
                                                       float* __restrict__ val_out, int d_sae, int k,
                                                       const int32_t* __restrict__ row_list, const uint32_t* __restrict__ n_list,
                                                       uint32_t* __restrict__ feat_cnt, uint32_t* __restrict__ wpos) {
    if (!row_list) {
        sae_topk_row(hidden, idx_out, val_out, d_sae, k, blockIdx.x, feat_cnt, wpos);
        return;
    }
    const uint32_t n = *n_list;
    for (uint32_t s = blockIdx.x; s < n; s += gridDim.x) {
        __syncthreads();
        sae_topk_row(hidden, idx_out, val_out, d_sae, k, row_list[s], feat_cnt, wpos);
    }
}

__device__ void sae_topk_row(const float* __restrict__ hidden, int32_t* __restrict__ idx_out, float* __restrict__ val_out,
                             int d_sae, int k, int64_t row, uint32_t* __restrict__ feat_cnt, uint32_t* __restrict__ wpos) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t cand_key[TOPK_CAP];
    __shared__ int32_t cand_idx[TOPK_CAP];
    sae_topk_row_lds(hidden, idx_out, val_out, d_sae, k, row, feat_cnt, wpos, hist, cand_key, cand_idx);      // (sae.hpp)
}

// ------------------------------------------------------------------------------------------------
// decode + LN-out + loss partial + dY + dh    (one wave per token)
// ------------------------------------------------------------------------------------------------
// A wave owns a token; lane l owns the 16-byte column groups 4 l + 256 i (i < V4: d_in <= 256 V4), so every gathered
// W_dec row is fetched as V4 16-byte loads per lane (1 KiB per wave-instruction), four rows in flight (ld4, dot4: sae_bwd.hpp).
// The CSR scan that rides in this launch as one more workgroup: ScanRole / scan_body_256 (sae_bwd.hpp).  Launched by sae_decode (below)
// alone; what each parameter means to a caller: the fields of SaeDecode (sae_bwd.hpp).
// MODE 0: the whole thing.  The feature-parallel step cuts it at the reconstruction: MODE 1 = this rank's PARTIAL
// reconstruction sum_s val_s W_dec[idx_s] only (written to sae_out, no b_dec, no LN-out); MODE 2 = everything behind it, the
// reconstruction summed over the ranks coming in through pre_sum.
#ifndef PV_DEC_ROWS
#define PV_DEC_ROWS 4
#endif
template <int V4, int MODE = 0>
__global__ __launch_bounds__(256) void sae_decode_kernel(
    const float* __restrict__ x, const float* __restrict__ W_dec, const float* __restrict__ b_dec,
    const int32_t* __restrict__ idx, const float* __restrict__ val, const float* __restrict__ mu,
    const float* __restrict__ sd, const float* __restrict__ norm, float* __restrict__ sae_out,
    float* __restrict__ dY, float* __restrict__ dh, float* __restrict__ loss_partial, int n_tok, int d, int k,
    float grad_scale /* 2 / (N_global * d_in) */, int want_grad, const float* __restrict__ inv_norm,
    const float* __restrict__ pre_sum = nullptr, const float* __restrict__ addend = nullptr, float dh_add = 0.f,
    const uint32_t* __restrict__ tok_cnt = nullptr, const uint32_t* __restrict__ gate = nullptr, const ScanRole scan = ScanRole{}) {
    // scan.cnt != NULL: the launch carries one more workgroup than the tokens need, and that one runs the CSR scan (scan_body_256)
    if (MODE != 1 && scan.cnt && blockIdx.x == gridDim.x - 1) {
        scan_body_256(scan);
        return;
    }
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= n_tok) return;
    if (gate && *gate != 0u) return;
    bool ok[V4];
    int col[V4];
#pragma unroll
    for (int i = 0; i < V4; ++i) {
        col[i] = 4 * lane + 256 * i;
        ok[i] = col[i] < d;
    }
    float4 acc[V4];
#pragma unroll
    for (int i = 0; i < V4; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    const int32_t* ir = idx + (int64_t)n * k;
    const float* vr = val + (int64_t)n * k;
    const int k_walk = tok_cnt ? min(k, (int)((tok_cnt[n] + 3u) & ~3u)) : k;       // (slots beyond it are holes)
    if constexpr (MODE == 2) {
#pragma unroll
        for (int i = 0; i < V4; ++i) acc[i] = ld4(pre_sum + (int64_t)n * d + col[i], ok[i]);
    }
    if (MODE == 0 && addend) {
#pragma unroll
        for (int i = 0; i < V4; ++i) acc[i] = ld4(addend + (int64_t)n * d + col[i], ok[i]);
    }
    // DEC_R rows of W_dec in flight per trip (k_walk is a multiple of 4; a trip that reaches past it gathers nothing for those slots: a = 0).
    // 4: 106 VGPRs = four waves per SIMD = all 4096 tokens of the bench batch resident at once.  8 halves the dependent trips and
    // costs a wave per SIMD: 66 -> 90 us (tools/probes/dec_rows_ab.sh, -DPV_DEC_ROWS=8; same bits)
    constexpr int DEC_R = PV_DEC_ROWS;
    for (int s = 0; MODE != 2 && s < k_walk; s += DEC_R) {
        float a[DEC_R];
        float4 w[DEC_R][V4];
#pragma unroll
        for (int u = 0; u < DEC_R; ++u) {
            const int su = min(s + u, k - 1);
            const int ju = ir[su];
            const float v = s + u < k_walk ? vr[su] : 0.f;
            a[u] = v > 0.f ? v : 0.f;                             // a value <= 0 is a hole (pv_native.h): a negative one the caller of
                                                                  // pv_sae_tp_partial / pv_sae_tp_finish hands over adds nothing either
            const bool live = a[u] != 0.f;                        // (wave-uniform) a hole -- a candidate that lost the global top-k of the
                                                                  // feature-parallel step, a clamped negative -- gathers nothing
            if (inv_norm) a[u] *= inv_norm[ju];
            const float* wr = W_dec + (int64_t)ju * d;
#pragma unroll
            for (int i = 0; i < V4; ++i) w[u][i] = ld4(wr + col[i], ok[i] && live);
        }
#pragma unroll
        for (int u = 0; u < DEC_R; ++u)                   // (slot order, as torch's dense matmul would not care; fixed here)
#pragma unroll
            for (int i = 0; i < V4; ++i) {
                acc[i].x += a[u] * w[u][i].x; acc[i].y += a[u] * w[u][i].y;
                acc[i].z += a[u] * w[u][i].z; acc[i].w += a[u] * w[u][i].w;
            }
    }
    if constexpr (MODE == 1) {
#pragma unroll
        for (int i = 0; i < V4; ++i)
            if (ok[i]) *reinterpret_cast<float4*>(sae_out + (int64_t)n * d + col[i]) = acc[i];
        return;
    }
    const float m = mu[n], sdv = sd[n], nf = norm[n];
    float lsum = 0.f;
    float4 g[V4];
#pragma unroll
    for (int i = 0; i < V4; ++i) {
        g[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok[i]) {
            const float4 bd = *reinterpret_cast<const float4*>(b_dec + col[i]);
            const float4 xv = *reinterpret_cast<const float4*>(x + (int64_t)n * d + col[i]);
            float4 o, e;
            o.x = (acc[i].x + bd.x) * sdv + m; o.y = (acc[i].y + bd.y) * sdv + m;      // decode (sae.py:583-595) + LN-out (:89-90)
            o.z = (acc[i].z + bd.z) * sdv + m; o.w = (acc[i].w + bd.w) * sdv + m;
            e.x = o.x - xv.x; e.y = o.y - xv.y; e.z = o.z - xv.z; e.w = o.w - xv.w;
            if (sae_out) *reinterpret_cast<float4*>(sae_out + (int64_t)n * d + col[i]) = o;
            lsum += (e.x * e.x) / nf + (e.y * e.y) / nf + (e.z * e.z) / nf + (e.w * e.w) / nf;      // sae.py:146-148
            g[i].x = grad_scale * e.x / nf * sdv; g[i].y = grad_scale * e.y / nf * sdv;            // dL/d(pre-LN-out reconstruction)
            g[i].z = grad_scale * e.z / nf * sdv; g[i].w = grad_scale * e.w / nf * sdv;
            if (want_grad) *reinterpret_cast<float4*>(dY + (int64_t)n * d + col[i]) = g[i];
        }
    }
    lsum = wave_sum(lsum);
    if (lane == 0) loss_partial[n] = lsum;
    if (!want_grad) return;
    for (int s = 0; s < k_walk; s += DEC_R) {
        float dot[DEC_R];
#pragma unroll
        for (int u = 0; u < DEC_R; ++u) {
            const int su = min(s + u, k - 1);
            const int ju = ir[su];
            const bool live = s + u < k_walk && vr[su] > 0.f;     // (wave-uniform) dh of a hole is gated to 0 below: no gather
            const float* wr = W_dec + (int64_t)ju * d;
            float t = 0.f;
#pragma unroll
            for (int i = 0; i < V4; ++i) t += dot4(g[i], ld4(wr + col[i], ok[i] && live));
            dot[u] = inv_norm ? t * inv_norm[ju] : t;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
#pragma unroll
            for (int u = 0; u < DEC_R; ++u) dot[u] += __shfl_xor(dot[u], o, 64);
        // TopK backward: gradient reaches only selected entries; ReLU gate on the kept value
        if (lane < DEC_R && s + lane < k && s + lane < ((k_walk + 3) & ~3)) {
            float dsel = dot[0];
#pragma unroll
            for (int u = 1; u < DEC_R; ++u) dsel = lane == u ? dot[u] : dsel;
            dh[(int64_t)n * k + s + lane] = vr[s + lane] > 0.f ? dsel + dh_add : 0.f;
        }
    }
}

// deterministic scalar reduction: out[slot] = scale * sum(v[0..n))
__global__ __launch_bounds__(256) void reduce_sum_kernel(const float* __restrict__ v, float* __restrict__ out, int n,
                                                         float scale, int slot, int slot2, const uint32_t* __restrict__ gate = nullptr,
                                                         uint32_t want = 0u) {
    __shared__ float red[4];
    if (gate && *gate != want) return;                          // (pv_sae_relu_step: only in the mode this sum belongs to)
    // (a fixed order -- the result is run-to-run identical --, four accumulators over 16-byte loads: the one workgroup reduces up to
    // 24 576 partials, and 96 dependent 4-byte loads per thread made each of the dense steps' four reductions 12 us)
    float s;
    if ((n & 3) == 0 && (reinterpret_cast<uintptr_t>(v) & 15) == 0) {
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        for (int i = threadIdx.x * 4; i < n; i += 1024) {
            const float4 t = *reinterpret_cast<const float4*>(v + i);
            s0 += t.x; s1 += t.y; s2 += t.z; s3 += t.w;
        }
        s = (s0 + s1) + (s2 + s3);
    } else {
        s = 0.f;
        for (int i = threadIdx.x; i < n; i += 256) s += v[i];
    }
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) {
        out[slot] = s * scale;
        if (slot2 >= 0) out[slot2] = s * scale;
    }
}

// The step's last launch with the clip norm in it (PV_SAE_FUSED_SQNORM).  Workgroup b of the nb that finish gb_dec (64 columns each)
// also takes block b of the clip norm: the squares of its own 64 columns + the b-th of nb slices of the backward's per-feature terms
// (rowsq) -> sqpart[b]; the workgroup that finishes LAST (a ticket from an agent-scope acq_rel counter; the partials travel as
// agent-scope atomics, so no cache of another XCD can hold a stale one) adds the nb partials in block order -> scalars[3] and re-arms
// the counter.  The sum is a fixed function of the inputs: which workgroup comes last does not enter it.  sq_block_terms is that
// block's arithmetic, shared with the one-workgroup form (sqnorm_blocks_kernel: the same bits from a launch of its own).
__device__ __forceinline__ float sq_block_terms(int b, int nb, float g, const float* __restrict__ rowsq, int d_sae, float* red16) {
    // g: this thread's column of block b (threads of wave 0; 0 elsewhere)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int slice = (d_sae + nb - 1) / nb, lo = b * slice, hi = min(lo + slice, d_sae);
    float sr = 0.f;
    for (int j = lo + (int)threadIdx.x; j < hi; j += 1024) sr += rowsq[j];
    sr = wave_sum(sr);
    const float gg = wave_sum(g * g);                        // (only wave 0's matters)
    __syncthreads();
    if (lane == 0) red16[wv] = sr;
    __syncthreads();
    float t = 0.f;
    if (threadIdx.x == 0) {
        for (int w = 0; w < 16; ++w) t += red16[w];          // fixed order
        t += gg;
    }
    return t;                                                // (thread 0)
}
__global__ __launch_bounds__(1024) void colsum_final_sq_kernel(const float* __restrict__ partial, float* __restrict__ out, int nblk, int d,
                                                               const float* __restrict__ rowsq, int d_sae, float* __restrict__ sqpart,
                                                               uint32_t* __restrict__ ticket, float* __restrict__ scalars) {
    __shared__ float red16[16];
    const int b = blockIdx.x, nb = gridDim.x;
    const float g = colsum_final_body(b, partial, out, nblk, d, 1.0f);
    const float t = sq_block_terms(b, nb, g, rowsq, d_sae, red16);
    __shared__ uint32_t last;
    if (threadIdx.x == 0) {
        __hip_atomic_store(&sqpart[b], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t mine = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        last = mine == (uint32_t)nb - 1u ? 1u : 0u;
    }
    __syncthreads();
    if (last && threadIdx.x < 64) {
        // lane i fetches partial i (one memory round trip for all of them: read one after the other by one thread they were most of
        // this launch's time), lane 0 adds them in block order (nb <= 64: d_in <= 4096)
        const int lane = threadIdx.x;
        const float mine = lane < nb ? __hip_atomic_load(&sqpart[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
        float total = 0.f;
        for (int i = 0; i < nb; ++i) total += __shfl(mine, i, 64);
        if (lane == 0) {
            scalars[3] = total;
            __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}
// the same sum from a launch of its own (gb_dec finished by the launch before): one workgroup walks the blocks
__global__ __launch_bounds__(1024) void sqnorm_blocks_kernel(const float* __restrict__ gb_dec, int d, const float* __restrict__ rowsq,
                                                             int d_sae, float* __restrict__ scalars) {
    __shared__ float red16[16];
    const int nb = (d + 63) / 64;
    float total = 0.f;
    for (int b = 0; b < nb; ++b) {
        const int c = b * 64 + (int)threadIdx.x;
        const float g = (threadIdx.x < 64 && c < d) ? gb_dec[c] : 0.f;
        total += sq_block_terms(b, nb, g, rowsq, d_sae, red16);
    }
    if (threadIdx.x == 0) scalars[3] = total;
}

// gb_dec = colsum(dY) - W_enc gb_enc (the encoder-input path of b_dec: sae_in = x - b_dec).  The second term as partial rows
// for colsum_final_kernel, stacked under the dY partials with the sign folded in: workgroup c sums -gb_enc[j] * W_encT[j][:]
// over its GBD_ROWS features, skipping the features no token kept (gb_enc = 0: half of them on the bench batch), so the
// pass reads the fired rows of W_encT once, coalesced, instead of all of W_enc.
constexpr int GBD_ROWS = 96;
__device__ __forceinline__ void gbdec_partial_body(int bid, const float* __restrict__ W_encT, const float* __restrict__ gb_enc,
                                                   float* __restrict__ partial, int d_sae, int d) {
    __shared__ float red[3][1280];                       // waves 1..3 -> wave 0, up to 1280 columns (d_in <= 256 * 5)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int j0 = bid * GBD_ROWS, j1 = min(j0 + GBD_ROWS, d_sae);
    float4 acc[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    // (four of the wave's rows in flight: one row per trip was a chain of 24 dependent row fetches, the launch's whole 13 us; the rows
    // are still added in row order, a row no token kept is still neither read nor added)
    for (int jb = j0 + wv; jb < j1; jb += 16) {
        float g[4];
        float4 w[4][5];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = jb + 4 * u;
            g[u] = j < j1 ? gb_enc[j] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = jb + 4 * u;
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const int c = 4 * lane + 256 * i;
                w[u][i] = (g[u] != 0.f && c < d) ? *reinterpret_cast<const float4*>(W_encT + (int64_t)j * d + c) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (g[u] == 0.f) continue;                   // (wave-uniform)
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                if (4 * lane + 256 * i < d) {
                    acc[i].x -= g[u] * w[u][i].x; acc[i].y -= g[u] * w[u][i].y; acc[i].z -= g[u] * w[u][i].z; acc[i].w -= g[u] * w[u][i].w;
                }
            }
        }
    }
    if (wv > 0) {
#pragma unroll
        for (int i = 0; i < 5; ++i) *reinterpret_cast<float4*>(&red[wv - 1][4 * lane + 256 * i]) = acc[i];
    }
    __syncthreads();
    if (wv == 0) {
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const int c = 4 * lane + 256 * i;
            if (c < d) {
                float4 t = acc[i];
                for (int w = 0; w < 3; ++w) {            // fixed order
                    const float4 o = *reinterpret_cast<const float4*>(&red[w][c]);
                    t.x += o.x; t.y += o.y; t.z += o.z; t.w += o.w;
                }
                *reinterpret_cast<float4*>(partial + (int64_t)bid * d + c) = t;
            }
        }
    }
}
__global__ __launch_bounds__(256) void sae_gbdec_partial_kernel(const float* __restrict__ W_encT, const float* __restrict__ gb_enc,
                                                                float* __restrict__ partial, int d_sae, int d) {
    gbdec_partial_body(blockIdx.x, W_encT, gb_enc, partial, d_sae, d);
}

// 1 / ||W_dec[j]|| (the read-only half of set_decoder_norm_to_unit_norm): a wave takes four rows, all loads in flight
__global__ __launch_bounds__(256) void dec_inv_norm_kernel(const float* __restrict__ W, float* __restrict__ inv, int rows, int d) {
    const int lane = threadIdx.x & 63;
    const int j0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 4;
    if (j0 >= rows) return;
    float sq[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = 4 * lane; c < d; c += 256) {
        float4 w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) w[u] = ld4(W + (int64_t)min(j0 + u, rows - 1) * d + c, true);
#pragma unroll
        for (int u = 0; u < 4; ++u) sq[u] += w[u].x * w[u].x + w[u].y * w[u].y + w[u].z * w[u].z + w[u].w * w[u].w;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int u = 0; u < 4; ++u) sq[u] += __shfl_xor(sq[u], o, 64);
    if (lane < 4 && j0 + lane < rows) {
        const float s = lane == 0 ? sq[0] : (lane == 1 ? sq[1] : (lane == 2 ? sq[2] : sq[3]));
        inv[j0 + lane] = 1.0f / sqrtf(s);
    }
}

}  // namespace

void sae_topk_rows(const float* hidden, int32_t* idx_out, float* val_out, int d_sae, int k, int n_rows, const int32_t* row_list,
                   const uint32_t* n_list, int slots, uint32_t* feat_cnt, uint32_t* wpos, hipStream_t stream) {
    hipLaunchKernelGGL(sae_topk_kernel, dim3(row_list ? slots : n_rows), dim3(256), 0, stream, hidden, idx_out, val_out, d_sae, k,
                       row_list, n_list, feat_cnt, wpos);
}

// The one launch site of sae_decode_kernel: a token per wave, + the workgroup of the folded CSR scan when a.scan is set
int sae_decode(const SaeDecode& a, hipStream_t stream) {
    const bool scan = a.mode != 1 && a.scan.cnt;
    const dim3 grid((a.N + 3) / 4 + (scan ? 1 : 0)), block(256);
#define DECODE(D, MODE)                                                                                                              \
    hipLaunchKernelGGL((sae_decode_kernel<D, MODE>), grid, block, 0, stream, a.x, a.W_dec, a.b_dec, a.idx, a.val, a.mu, a.sd, a.norm, \
                       a.sae_out, a.dY, a.dh, a.loss_part, a.N, a.d, a.k, a.grad_scale, a.dY ? 1 : 0, a.inv_norm, a.pre_sum, a.addend, \
                       a.dh_add, a.tok_cnt, a.gate, a.scan)
#define CALL(D)                                  \
    do {                                         \
        if (a.mode == 0) DECODE(D, 0);           \
        else if (a.mode == 1) DECODE(D, 1);      \
        else DECODE(D, 2);                       \
    } while (0)
    V4_DISPATCH(a.d, CALL);
#undef CALL
#undef DECODE
    PV_LAUNCH_CHECK("sae_decode_kernel");
    return PV_OK;
}

// ------------------------------------------------------------------------------------------------
// plan + C ABI
// ------------------------------------------------------------------------------------------------
SaeWs sae_carve(const pv_sae_desc& d) {
    SaeWs w;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (size_t)pv_align_up((int64_t)bytes, 256); return o; };
    const size_t N = d.max_tokens;
    w.sq_blocks = 1024;
    w.hidden = take(N * (size_t)d.d_sae * 4);        // exact path: hidden_pre; filtered path: rows of undecided tokens only
    w.sae_in = take(N * (size_t)d.d_in * 4);
    w.dY = take(N * (size_t)d.d_in * 4);
    w.mu = take(N * 4);
    w.sd = take(N * 4);
    w.norm = take(N * 4);
    w.dh = take(N * (size_t)d.k * 4);
    w.loss_part = take(N * 4);
    w.cnt = take((size_t)d.d_sae * 4);
    w.offs = take(((size_t)d.d_sae + 1) * 4);
    w.cursor = take((N * (size_t)d.k / BWD_CH + 8) * 4);      // chunk starts of the backward's waves
    w.wpos = take(N * (size_t)d.k * 4);
    w.long_list = take((size_t)d.d_sae * 12);
    w.n_long = take(256);
    {
        const size_t max_segs = sae_max_segs(N * (size_t)d.k);
        w.seg_range = take(max_segs * 8);
        w.seg_rows = take(max_segs * 2 * (size_t)d.d_in * 4);
        w.seg_b = take(max_segs * 4);
    }
    w.pairs = take(N * (size_t)d.k * 4);
    w.colpart = take((size_t)((d.max_tokens + CS_ROWS - 1) / CS_ROWS + (d.d_sae + GBD_ROWS - 1) / GBD_ROWS) * d.d_in * 4);
    w.colsum = take((size_t)d.d_in * 4);
    w.batch_mean = take((size_t)d.d_in * 4);
    w.sqpart = take((size_t)w.sq_blocks * 4);
    w.rowsq = take((size_t)d.d_sae * 4);              // per-feature terms of the clip norm (backward kernels)
    w.x16 = take(N * (size_t)d.d_in * 2);
    w.xnorm = take(N * 4);
    w.sample = take(N * (size_t)(d.d_sae / PV_SAE_SAMPLE_STRIDE + 1) * 4);
    w.thr = take(N * 4);
    w.sq = take(N * 4);
    w.band = take(N * 4);
    const size_t ntn = (size_t)(d.d_sae + 255) / 256;
    w.cand_cnt = take(N * ntn * 4);
    w.cand = take(N * ntn * (size_t)pv_sae_tile_slots(d) * 8);
    w.fb_list = take(N * 4);
    w.fb_count = take(256);
    w.wmax = take(256);
    {   // dense (ReLU + L1) step, sae_dense.hip
        const size_t rblk = (N + 63) / 64, cblk = ((size_t)d.d_sae + 63) / 64;
        w.dense_colpart = take(rblk * (size_t)d.d_sae * 4);
        w.dense_rowpart = take(rblk * cblk * 4);
        w.dense_kpart = take((size_t)PV_SAE_DENSE_SPLITK * N * (size_t)d.d_in * 4);
        w.dense_amax = take((size_t)PV_SAE_AMAX_TENSORS * 256 * 4);
        const bool lp = d.lp_norm != 0.f && d.lp_norm != 1.f;
        w.dense_lp_part = take(lp ? N * cblk * 4 : 0);
        w.dense_lp_tok = take(lp ? N * 4 : 0);
        w.dense_lp_loss = take(lp ? N * 4 : 0);
    }
    w.total = off + 256;
    return w;
}

// The buffers of the sparse ReLU + L1 step that depend on its per-token capacity (pv_sae_relu_step; caller-owned workspace)
ReluWs relu_carve(const pv_sae_desc& d, int n_tokens, int cap) {
    ReluWs w;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (size_t)pv_align_up((int64_t)bytes, 256); return o; };
    const size_t N = (size_t)n_tokens, P = N * (size_t)cap, ntn = (size_t)(d.d_sae + 255) / 256;
    w.mode = take(256);
    w.idx = take(P * 4);
    w.val = take(P * 4);
    w.tok_cnt = take(N * 4);
    w.l1part = take(N * 4);
    w.cand_cnt = take(N * ntn * 4);
    w.cand = take(N * ntn * (size_t)PV_SAE_RELU_SLOTS * 8);
    w.dh = take(P * 4);
    w.cursor = take((P / BWD_CH + 8) * 4);
    w.wpos = take(P * 4);
    w.max_segs = (int)sae_max_segs(P);
    w.seg_range = take((size_t)w.max_segs * 8);
    w.seg_rows = take((size_t)w.max_segs * 2 * (size_t)d.d_in * 4);
    w.seg_b = take((size_t)w.max_segs * 4);
    w.pairs = take(P * 4);
    w.total = off + 256;
    return w;
}

extern "C" int pv_sae_plan_create(const pv_sae_desc* desc, pv_sae_plan** out_plan) {
    PV_REQUIRE(desc && out_plan, "null argument");
    PV_REQUIRE(desc->d_in > 1 && desc->d_in <= 64 * 20 && desc->d_in % 4 == 0, "d_in must be a multiple of 4, <= 1280 (ViT-H/14)");
    PV_REQUIRE(desc->d_sae >= desc->k && desc->d_sae % 4 == 0 && desc->d_sae <= 256 * 256, "d_sae must be a multiple of 4, <= 65536");
    // (k <= 64: the filtered encoder; beyond it, up to 256, the exact fp32 encoder + the streaming top-k serve the plan -- pv_sae_fast_ok)
    PV_REQUIRE(desc->k >= 1 && desc->k <= 256, "k must be in [1, 256]");
    PV_REQUIRE(desc->max_tokens >= 1, "max_tokens");
    PV_REQUIRE(desc->normalize_layer_norm >= 0 && desc->normalize_layer_norm <= 2, "normalize_layer_norm: 0 none, 1 layer_norm, 2 constant_norm_rescale");
    PV_REQUIRE(desc->activation == PV_SAE_ACT_RELU || desc->activation == PV_SAE_ACT_TANH_RELU, "activation: PV_SAE_ACT_RELU or PV_SAE_ACT_TANH_RELU");
    PV_REQUIRE(desc->lp_norm == 0.f || desc->lp_norm >= 1.f, "lp_norm: 0 / 1 (the 1-norm) or p > 1 (p < 1 has no finite gradient at zero activations)");
    pv_sae_plan* p = new pv_sae_plan();
    p->d = *desc;
    *out_plan = p;
    return PV_OK;
}
extern "C" void pv_sae_plan_destroy(pv_sae_plan* plan) { delete plan; }
extern "C" size_t pv_sae_workspace_bytes(const pv_sae_plan* plan) { return plan ? sae_carve(plan->d).total : 0; }
extern "C" int pv_sae_encoder_is_filtered(const pv_sae_plan* plan) { return plan && pv_sae_fast_ok(plan->d) ? 1 : 0; }
// debug / tests: byte offset of a named region of the workspace ("fb_count": uint32 number of tokens of the last encode that
// took the exact fallback; "cand_cnt": uint32 [N] candidates per token), or (size_t)-1
extern "C" size_t pv_debug_sae_ws_offset(const pv_sae_plan* plan, const char* name) {
    if (!plan || !name) return (size_t)-1;
    const SaeWs w = sae_carve(plan->d);
    if (!strcmp(name, "fb_count")) return w.fb_count;
    if (!strcmp(name, "fb_list")) return w.fb_list;
    if (!strcmp(name, "cand_cnt")) return w.cand_cnt;
    if (!strcmp(name, "thr")) return w.thr;
    if (!strcmp(name, "hidden")) return w.hidden;
    if (!strcmp(name, "dY")) return w.dY;
    if (!strcmp(name, "sae_in")) return w.sae_in;
    if (!strcmp(name, "dense_amax")) return w.dense_amax;          // PV_SAE_AMAX_TENSORS x 256 uint32 (bit patterns of partial maxima)
    return (size_t)-1;
}

// ---- transcoder (pv_sae_state.tc; sae/transcoder.py:6-116) ----------------------------------------------------------------
// loss normaliser of the target: ||y_n - mean_n(y)||_2 (sae.py:145-147 as called by transcoder.py:78).  One wave per token.
// d_true < d (a transcoder whose output is narrower than its input, pv_sae_transcoder.d_out_true: rows padded to the common width d):
// the norm runs over the real columns, and the padding of the target row is set to the token's LN mean -- exactly what the decoder
// (zero padded columns of W_dec / b_dec_out) reconstructs there after LN-out, so that the padding's error, loss and gradient are exact
// zeros
__global__ __launch_bounds__(256) void sae_target_norm_kernel(float* __restrict__ y, const float* __restrict__ batch_mean,
                                                              float* __restrict__ norm_out, int n_tok, int d, int d_true,
                                                              const float* __restrict__ mu) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= n_tok) return;
    float cn = 0.f;
    for (int i = lane; i < d_true; i += 64) {
        const float c = y[(int64_t)n * d + i] - batch_mean[i];
        cn += c * c;
    }
    cn = wave_sum(cn);
    if (lane == 0) norm_out[n] = sqrtf(cn);
    for (int i = d_true + lane; i < d; i += 64) y[(int64_t)n * d + i] = mu[n];
}

int sae_tc_require(const pv_sae_desc& d, const pv_sae_state* st, int N) {
    const pv_sae_transcoder& t = st->tc;
    PV_REQUIRE(t.b_dec_out && t.gb_dec_out && t.target, "transcoder state: b_dec_out, gb_dec_out and target are required");
    const bool any_skip = t.W_skip || t.gW_skip;
    PV_REQUIRE(!any_skip || (t.W_skip && t.gW_skip), "transcoder state: W_skip and gW_skip come together");
    PV_REQUIRE(t.d_in_true >= 0 && t.d_in_true <= d.d_in && t.d_out_true >= 0 && t.d_out_true <= d.d_in &&
                   (t.d_in_true == 0 || t.d_in_true == d.d_in || t.d_out_true == 0 || t.d_out_true == d.d_in),
               "transcoder widths: d_in_true / d_out_true are 0 (= the plan's d_in) or the real widths of rows padded to max(d_in, d_out)");
    PV_REQUIRE(!t.W_skip || ((t.d_in_true == 0 || t.d_in_true == d.d_in) && (t.d_out_true == 0 || t.d_out_true == d.d_in)),
               "the skip connection needs d_out == d_in (transcoder.py:10, 73-76)");
    if (t.W_skip) {
        PV_REQUIRE(d.d_in % 8 == 0, "the skip connection's GEMMs need d_in to be a multiple of 8");
        PV_REQUIRE(t.scratch && ((uintptr_t)t.scratch & 255) == 0 &&
                       t.scratch_bytes >= ((size_t)N * d.d_in + (size_t)PV_SAE_SKIP_SPLITK * d.d_in * d.d_in) * 4,
                   "transcoder scratch too small / misaligned (pv_sae_transcoder_scratch_bytes)");
    }
    return PV_OK;
}

extern "C" size_t pv_sae_transcoder_scratch_bytes(const pv_sae_plan* plan, int32_t n_tokens) {
    if (!plan || n_tokens < 1) return 0;
    const pv_sae_desc& d = plan->d;
    return (size_t)pv_align_up((int64_t)(((size_t)n_tokens * d.d_in + (size_t)PV_SAE_SKIP_SPLITK * d.d_in * d.d_in) * 4), 256);
}

int sae_tc_target_norm(const pv_sae_desc& d, const pv_sae_state* st, const float* batch_mean, int N, unsigned char* wsb, const SaeWs& ws,
                       hipStream_t stream) {
    float* bmean = (float*)(wsb + ws.batch_mean);
    const float* y = st->tc.target;
    if (batch_mean) {
        PV_HIP_CHECK(hipMemcpyAsync(bmean, batch_mean, (size_t)d.d_in * 4, hipMemcpyDeviceToDevice, stream));
    } else {
        const int nblk = (N + CS_ROWS - 1) / CS_ROWS;
        hipLaunchKernelGGL(colsum_partial_kernel, dim3(nblk), dim3(256), 0, stream, y, (float*)(wsb + ws.colpart), N, d.d_in);
        hipLaunchKernelGGL(colsum_final_kernel, dim3((d.d_in + 63) / 64), dim3(1024), 0, stream,
                           (const float*)(wsb + ws.colpart), bmean, nblk, d.d_in, 1.0f / (float)N);
    }
    hipLaunchKernelGGL(sae_target_norm_kernel, dim3((N + 3) / 4), dim3(256), 0, stream, const_cast<float*>(y), (const float*)bmean,
                       (float*)(wsb + ws.norm), N, d.d_in, sae_loss_width(d, st), (const float*)(wsb + ws.mu));
    PV_LAUNCH_CHECK("sae_target_norm_kernel");
    return PV_OK;
}

// ---- pieces of the step shared with the dense (ReLU + L1) step of sae_dense.hip --------------------------------------------
// batch mean (given, or computed from x) -> ws.batch_mean; LN-in, sae_in, loss normaliser (+ the fp16 copy / row norms the
// filtered encoder wants) -> ws.sae_in, ws.mu, ws.sd, ws.norm (ws.x16, ws.xnorm)
int sae_prep(const pv_sae_desc& d, const float* x, const float* b_dec, const float* batch_mean, int N, bool want_filter_inputs,
             unsigned char* wsb, const SaeWs& ws, hipStream_t stream, int d_true, SaePre* pre, const pv_sae_state* st, uint32_t* feat_cnt) {
    float* bmean = (float*)(wsb + ws.batch_mean);
    const int nblk = (N + CS_ROWS - 1) / CS_ROWS;
    if (batch_mean) PV_HIP_CHECK(hipMemcpyAsync(bmean, batch_mean, (size_t)d.d_in * 4, hipMemcpyDeviceToDevice, stream));
    if (pre) {                                                   // the fused pre-pass (SaePre): one launch, the mean and the normaliser come later
        pre->x = x; pre->d_true = d_true > 0 ? d_true : d.d_in; pre->have_mean = batch_mean != nullptr;
        const int nb_prep = (N + 3) / 4, nb_cs = batch_mean ? 0 : nblk;
        hipLaunchKernelGGL(sae_prep_roles_kernel, dim3(nb_prep + nb_cs + 1), dim3(256), 0, stream, x, b_dec, (float*)(wsb + ws.sae_in),
                           (_Float16*)(wsb + ws.x16), (float*)(wsb + ws.xnorm), (float*)(wsb + ws.mu), (float*)(wsb + ws.sd), N, d.d_in,
                           d.normalize_layer_norm, d.ln_eps, pre->d_true, nb_prep, (float*)(wsb + ws.colpart), nb_cs,
                           (const float*)st->enc_colsq, d.d_sae, (float*)(wsb + ws.wmax), (uint32_t*)(wsb + ws.fb_count), feat_cnt);
        PV_LAUNCH_CHECK("sae_prep_roles_kernel");
        return PV_OK;
    }
    if (!batch_mean) {
        hipLaunchKernelGGL(colsum_partial_kernel, dim3(nblk), dim3(256), 0, stream, x, (float*)(wsb + ws.colpart), N, d.d_in);
        hipLaunchKernelGGL(colsum_final_kernel, dim3((d.d_in + 63) / 64), dim3(1024), 0, stream,
                           (const float*)(wsb + ws.colpart), bmean, nblk, d.d_in, 1.0f / (float)N);
    }
    hipLaunchKernelGGL(sae_prep_kernel, dim3((N + 3) / 4), dim3(256), 0, stream, x, b_dec, (const float*)bmean,
                       (float*)(wsb + ws.sae_in), want_filter_inputs ? (_Float16*)(wsb + ws.x16) : (_Float16*)nullptr,
                       want_filter_inputs ? (float*)(wsb + ws.xnorm) : (float*)nullptr, (float*)(wsb + ws.mu), (float*)(wsb + ws.sd),
                       (float*)(wsb + ws.norm), N, d.d_in, d.normalize_layer_norm, d.ln_eps, d_true > 0 ? d_true : d.d_in);
    PV_LAUNCH_CHECK("sae_prep_kernel");
    return PV_OK;
}

// The bias gradients behind every step: colsum(dY) and the encoder-input path of b_dec, -W_enc @ gb_enc, both as partial rows of a column
// sum (ws.colpart: nblk rows of dY partials, under them the ngb rows of sae_gbdec_partial_kernel).  dy_to: which parameter colsum(dY)
// belongs to (SaeDyTo, sae.hpp).  have_colsum: the partial column sums of dY are in ws.colpart already (csr_post_fill_kernel).
int sae_gbdec(const pv_sae_desc& d, const pv_sae_state* st, const float* dY, int N, unsigned char* wsb, const SaeWs& ws,
              hipStream_t stream, SaeDyTo dy_to, bool have_colsum, float* sq_scalars) {
    const int nblk = (N + CS_ROWS - 1) / CS_ROWS, ngb = (d.d_sae + GBD_ROWS - 1) / GBD_ROWS;
    const dim3 grid_fin((d.d_in + 63) / 64), block_fin(1024);
    float* colpart = (float*)(wsb + ws.colpart);
    float* encpart = colpart + (size_t)nblk * d.d_in;
    if (!have_colsum) hipLaunchKernelGGL(colsum_partial_kernel, dim3(nblk), dim3(256), 0, stream, dY, colpart, N, d.d_in);
    hipLaunchKernelGGL(sae_gbdec_partial_kernel, dim3(ngb), dim3(256), 0, stream, (const float*)st->W_encT, (const float*)st->gb_enc,
                       encpart, d.d_sae, d.d_in);
    if (dy_to == SAE_DY_TO_GB_DEC_OUT)
        hipLaunchKernelGGL(colsum_final_kernel, grid_fin, block_fin, 0, stream, (const float*)colpart, st->tc.gb_dec_out, nblk, d.d_in, 1.0f);
    if (dy_to != SAE_DY_TO_GB_DEC)  // the encoder term alone
        hipLaunchKernelGGL(colsum_final_kernel, grid_fin, block_fin, 0, stream, (const float*)encpart, st->gb_dec, ngb, d.d_in, 1.0f);
    else if (sq_scalars)            // PV_SAE_FUSED_SQNORM: the clip norm out of the same launch (the ticket word: n_long[2], zeroed by the scan)
        hipLaunchKernelGGL(colsum_final_sq_kernel, grid_fin, block_fin, 0, stream, (const float*)colpart, st->gb_dec,
                           nblk + ngb, d.d_in, (const float*)(wsb + ws.rowsq), d.d_sae, (float*)(wsb + ws.sqpart),
                           (uint32_t*)(wsb + ws.n_long) + 2, sq_scalars);
    else
        hipLaunchKernelGGL(colsum_final_kernel, grid_fin, block_fin, 0, stream, (const float*)colpart, st->gb_dec, nblk + ngb, d.d_in, 1.0f);
    PV_LAUNCH_CHECK("sae bias-grad kernels");
    return PV_OK;
}

// out[c] = scale * sum_rows x[r][c] for a [rows][d] matrix; `partial` = (rows / 16 + 1) * d floats of scratch
int sae_colsum(const float* x, int rows, int d, float* out, float scale, float* partial, hipStream_t stream) {
    const int nblk = (rows + CS_ROWS - 1) / CS_ROWS;
    hipLaunchKernelGGL(colsum_partial_kernel, dim3(nblk), dim3(256), 0, stream, x, partial, rows, d);
    hipLaunchKernelGGL(colsum_final_kernel, dim3((d + 63) / 64), dim3(1024), 0, stream, (const float*)partial, out, nblk, d, scale);
    PV_LAUNCH_CHECK("colsum kernels");
    return PV_OK;
}

// out[slot] (and out[slot2] when >= 0) = scale * sum(v[0..n)), one workgroup, fixed order
void sae_reduce_sum(const float* v, float* out, int n, float scale, int slot, int slot2, hipStream_t stream, const uint32_t* gate,
                    uint32_t want) {
    hipLaunchKernelGGL(reduce_sum_kernel, dim3(1), dim3(256), 0, stream, v, out, n, scale, slot, slot2, gate, want);
}

// prep + encoder + top-k (the arguments: sae.hpp)
int sae_encode_topk(pv_sae_plan* plan, const pv_sae_state* st, const float* x, int N, const float* batch_mean,
                    int32_t* topk_idx, float* topk_val, bool want_csr, unsigned char* wsb, const SaeWs& ws, hipStream_t stream,
                    uint32_t* cnt_over, uint32_t* wpos_over, bool skip_prep) {
    const pv_sae_desc& d = plan->d;
    uint32_t* feat_cnt = want_csr ? (cnt_over ? cnt_over : (uint32_t*)(wsb + ws.cnt)) : nullptr;
    uint32_t* wpos = want_csr ? (wpos_over ? wpos_over : (uint32_t*)(wsb + ws.wpos)) : nullptr;
    const bool fast = pv_sae_fast_ok(d) && st->W_encT && st->W_enc16T && st->enc_colsq;
    if (want_csr && !fast) PV_HIP_CHECK(hipMemsetAsync(feat_cnt, 0, (size_t)d.d_sae * 4, stream));      // (fast path: its first kernel zeroes them)
    // the pre-pass in fused launches (SaePre)
    SaePre pre = {x, 0, false};
    const bool fused = fast && !skip_prep && !cnt_over && g_pv_tuning.sae_fold;      // (training steps, the feature-parallel encode, inference)
    if (!skip_prep) {
        int rcp = sae_prep(d, x, (const float*)st->b_dec, batch_mean, N, fast, wsb, ws, stream, sae_in_width(d, st), fused ? &pre : nullptr,
                           st, feat_cnt);
        if (rcp) return rcp;
    }
    // algorithmic work of the encoder: 2 N d_in d_sae FLOP; bytes = operands once (x, W_enc as fp16) + the k results
    ProfScope prof(PV_PROF_SAE_ENC, stream, 2.0 * N * (double)d.d_in * d.d_sae,
                   ((double)N * d.d_in + (double)d.d_in * d.d_sae) * (fast ? 2.0 : 4.0) + (double)N * d.k * 8.0 +
                       (fast ? 0.0 : (double)N * d.d_sae * 8.0));
    if (fast) return sae_encode_fast(d, st, N, topk_idx, topk_val, feat_cnt, wpos, wsb, ws, stream, fused ? &pre : nullptr);
    {
        // exact path: hidden_pre = sae_in @ W_enc + b_enc (sae.py:567-574) on the fp32 MFMA, W_enc in its own [d_in][d_sae] layout
        GemmParams g = {};
        g.A = wsb + ws.sae_in; g.lda = d.d_in; g.a_mode = PV_A_PLAIN;
        if (st->W_encT) { g.Bt = st->W_encT; g.ldb = d.d_in; g.b_kn = 0; }          // the transposed master (always current)
        else { g.Bt = st->W_enc; g.ldb = d.d_sae; g.b_kn = 1; }                      // no shadows: the parameter's own [K][N] layout
        g.M = N; g.N = d.d_sae; g.K = d.d_in; g.epi = PV_EPI_BIAS; g.bias0 = st->b_enc; g.out0 = wsb + ws.hidden; g.ldo = d.d_sae;
        int rc = pv_launch_gemm(PV_DTYPE_F32, g, stream);
        if (rc) return rc;
        sae_topk_rows((const float*)(wsb + ws.hidden), topk_idx, topk_val, d.d_sae, d.k, N, nullptr, nullptr, 0, feat_cnt, wpos, stream);
    }
    PV_LAUNCH_CHECK("sae_topk_kernel");
    return PV_OK;
}

extern "C" int pv_sae_encode_topk(pv_sae_plan* plan, const pv_sae_state* st, const float* x, int32_t N,
                                  int32_t* topk_idx, float* topk_val, float* ln_mu, float* ln_std, void* workspace,
                                  size_t workspace_bytes, void* stream_) {
    PV_REQUIRE(plan && st && x && topk_idx && topk_val && workspace, "null argument");
    PV_REQUIRE(N >= 1 && N <= plan->d.max_tokens, "n_tokens exceeds plan max_tokens");
    const SaeWs ws = sae_carve(plan->d);
    PV_REQUIRE(workspace_bytes >= ws.total, "workspace too small");
    hipStream_t stream = (hipStream_t)stream_;
    unsigned char* wsb = (unsigned char*)workspace;
    int rc = sae_encode_topk(plan, st, x, N, nullptr, topk_idx, topk_val, false, wsb, ws, stream);
    if (rc) return rc;
    if (ln_mu) PV_HIP_CHECK(hipMemcpyAsync(ln_mu, wsb + ws.mu, (size_t)N * 4, hipMemcpyDeviceToDevice, stream));
    if (ln_std) PV_HIP_CHECK(hipMemcpyAsync(ln_std, wsb + ws.sd, (size_t)N * 4, hipMemcpyDeviceToDevice, stream));
    return PV_OK;
}

// Inference forward of the module API (StandardSparseAutoencoder.forward / encode + decode, sae.py:557-645): top-k
// encode + sparse decode + LN-out -> sae_out [N, d_in]; no gradients, no statistics.  scalars[1] (optional) receives the
// mse loss over these N tokens taken as ONE batch (sae.py:144-149).
extern "C" int pv_sae_forward(pv_sae_plan* plan, const pv_sae_state* st, const float* x, int32_t N, float* sae_out,
                              int32_t* topk_idx, float* topk_val, float* ln_mu, float* ln_std, float* scalars, void* workspace,
                              size_t workspace_bytes, void* stream_) {
    PV_REQUIRE(!st || !sae_is_gated(st), "this entry point does not serve a gated state (pv_sae_state.gt)");
    PV_REQUIRE(!st || !sae_is_tc(st), "pv_sae_forward: not available for a transcoder state (pv_sae_state.tc)");
    PV_REQUIRE(plan && st && x && sae_out && topk_idx && topk_val && workspace, "null argument");
    const pv_sae_desc& d = plan->d;
    PV_REQUIRE(N >= 1 && N <= d.max_tokens, "n_tokens exceeds plan max_tokens");
    const SaeWs ws = sae_carve(d);
    PV_REQUIRE(workspace_bytes >= ws.total, "workspace too small");
    hipStream_t stream = (hipStream_t)stream_;
    unsigned char* wsb = (unsigned char*)workspace;
    int rc = sae_encode_topk(plan, st, x, N, nullptr, topk_idx, topk_val, false, wsb, ws, stream);
    if (rc) return rc;
    SaeDecode dec;                                                  // (no dY: decode, LN-out and the loss terms only)
    dec.N = N; dec.d = d.d_in; dec.k = d.k; dec.x = x; dec.W_dec = st->W_dec; dec.b_dec = st->b_dec; dec.idx = topk_idx; dec.val = topk_val;
    dec.mu = (const float*)(wsb + ws.mu); dec.sd = (const float*)(wsb + ws.sd); dec.norm = (const float*)(wsb + ws.norm);
    dec.sae_out = sae_out; dec.loss_part = (float*)(wsb + ws.loss_part);
    rc = sae_decode(dec, stream);
    if (rc) return rc;
    if (scalars)
        hipLaunchKernelGGL(reduce_sum_kernel, dim3(1), dim3(256), 0, stream, (const float*)(wsb + ws.loss_part), scalars, N,
                           1.0f / ((float)N * (float)d.d_in), 1, -1);
    if (ln_mu) PV_HIP_CHECK(hipMemcpyAsync(ln_mu, wsb + ws.mu, (size_t)N * 4, hipMemcpyDeviceToDevice, stream));
    if (ln_std) PV_HIP_CHECK(hipMemcpyAsync(ln_std, wsb + ws.sd, (size_t)N * 4, hipMemcpyDeviceToDevice, stream));
    return PV_OK;
}

// Everything of the k-sparse step behind the selection: decode + LN-out + loss + dY + dh, the CSR by feature, the sparse backward,
// the bias gradients.  Shared by pv_sae_step (k = the plan's k) and by the sparse form of the ReLU + L1 step (pv_sae_relu_step:
// k = the per-token capacity, tok_cnt / dh_add / gate as described at SaeDecode; the k-dependent buffers come in through tb).
int sae_sparse_tail(pv_sae_plan* plan, pv_sae_state* st, const float* x, int N, int n_global, int k, const int32_t* topk_idx,
                    const float* topk_val, float* sae_out, float* scalars, float* fire_count, int update_stats, bool sparse,
                    const float* inv_norm, const SaeTail& tb, unsigned char* wsb, const SaeWs& ws, const float* y, const float* bdo,
                    const float* skip, bool tc, float dh_add, const uint32_t* tok_cnt, const uint32_t* gate, hipStream_t stream,
                    bool bias_grads, float* sq_scalars) {
    const pv_sae_desc& d = plan->d;
    const int n_pairs = N * k;
    int rc = PV_OK;
    float* dY = (float*)(wsb + ws.dY);
    float* dh = tb.dh;
    float* sae_in = (float*)(wsb + ws.sae_in);
    {
        ProfScope prof(PV_PROF_SAE_BWD, stream, 4.0 * n_pairs * (double)d.d_in * 2.0, 0.0);
        const float loss_scale = 1.0f / ((float)n_global * (float)sae_loss_width(d, st));
        // the CSR scan reads the selection's counts only -- it runs as one more workgroup of the decode launch (ScanRole).  (The sparse
        // form of the ReLU step on a batch that turns out dense: the scan walks counts nobody will use and writes scalars the dense
        // form overwrites -- as the scan's own launch did)
        const bool folded = g_pv_tuning.sae_fold != 0;
        SaeDecode dec;
        dec.N = N; dec.d = d.d_in; dec.k = k; dec.x = y; dec.W_dec = st->W_dec; dec.b_dec = bdo; dec.idx = topk_idx; dec.val = topk_val;
        dec.mu = (const float*)(wsb + ws.mu); dec.sd = (const float*)(wsb + ws.sd); dec.norm = (const float*)(wsb + ws.norm);
        dec.sae_out = sae_out; dec.dY = dY; dec.dh = dh; dec.loss_part = (float*)(wsb + ws.loss_part);
        dec.grad_scale = 2.0f / ((float)n_global * (float)sae_loss_width(d, st));      // (a transcoder: the mean is over N x d_out)
        dec.inv_norm = inv_norm; dec.addend = skip; dec.dh_add = dh_add; dec.tok_cnt = tok_cnt; dec.gate = gate;
        if (folded) dec.scan = sae_scan_role(d, wsb, ws, (const uint32_t*)(wsb + ws.cnt), scalars, N);
        rc = sae_decode(dec, stream);
        if (rc) return rc;
        const bool cs_here = bias_grads && !tc;
        SaeBwd b;
        b.N = N; b.k = k; b.idx = topk_idx; b.val = topk_val; b.dY = dY; b.sae_in = sae_in; b.scalars = scalars; b.tail = tb;
        b.fire_count = fire_count; b.update_stats = update_stats; b.sparse_grads = sparse; b.gate = gate;
        b.loss_part = (const float*)(wsb + ws.loss_part); b.loss_scale = loss_scale; b.colsum_dY = cs_here; b.folded = folded;
        rc = sae_csr_backward(plan, st, b, wsb, ws, stream);
        if (rc) return rc;
        // gb_dec = colsum(dY) - W_enc @ gb_enc: both terms as partial rows of one column sum
        // (bias_grads false: pv_sae_relu_step runs them once, behind whichever of its two forms produced dY and gb_enc)
        if (bias_grads) {
            rc = sae_gbdec(d, st, dY, N, wsb, ws, stream, tc ? SAE_DY_TO_GB_DEC_OUT : SAE_DY_TO_GB_DEC, cs_here, sq_scalars);
            if (rc) return rc;
            if (tc) {
                rc = sae_tc_skip_backward(d, st, x, dY, N, stream);
                if (rc) return rc;
            }
        }
    }
    return PV_OK;
}

int sae_dec_inv_norm(const pv_sae_desc& d, const pv_sae_state* st, hipStream_t stream) {
    hipLaunchKernelGGL(dec_inv_norm_kernel, dim3((d.d_sae + 15) / 16), dim3(256), 0, stream, (const float*)st->W_dec, st->dec_inv_norm,
                       d.d_sae, d.d_in);
    PV_LAUNCH_CHECK("dec_inv_norm_kernel");
    return PV_OK;
}

extern "C" int pv_sae_step(pv_sae_plan* plan, pv_sae_state* st, const float* x, int32_t N, const float* batch_mean,
                           int32_t n_global, int32_t flags, pv_sae_out* out, void* workspace,
                           size_t workspace_bytes, void* stream_) {
    const int update_stats = (flags & PV_SAE_UPDATE_STATS) ? 1 : 0;
    const bool renorm = (flags & PV_SAE_RENORM_DECODER) != 0;
    const bool sparse = (flags & PV_SAE_SPARSE_GRADS) != 0;
    const bool fused_sq = (flags & PV_SAE_FUSED_SQNORM) != 0;
    PV_REQUIRE(plan && st && x && out && workspace, "null argument");
    PV_REQUIRE(out->topk_idx && out->topk_val && out->scalars, "pv_sae_out buffers");
    PV_REQUIRE(!fused_sq || (st->tc.b_dec_out == nullptr && plan->d.d_in <= 4096),
               "PV_SAE_FUSED_SQNORM: autoencoder states of d_in <= 4096 (a transcoder's clip norm has more terms: pv_sae_grad_sqnorm_step)");
    PV_REQUIRE(st->W_dec && st->b_enc && st->b_dec && st->gW_enc && st->gW_dec && st->gb_enc && st->gb_dec, "state");
    PV_REQUIRE(st->W_encT, "pv_sae_step needs the transposed encoder copy (pv_sae_state.W_encT, see pv_sae_sync_shadows)");
    PV_REQUIRE(!update_stats || (st->act_freq_scores && st->n_fwd_since_fired), "stats buffers");
    const pv_sae_desc& d = plan->d;
    PV_REQUIRE(N >= 1 && N <= d.max_tokens, "n_tokens exceeds plan max_tokens");
    PV_REQUIRE(n_global >= N, "n_global must be >= n_tokens");
    const SaeWs ws = sae_carve(d);
    PV_REQUIRE(workspace_bytes >= ws.total, "workspace too small");
    PV_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace alignment");
    hipStream_t stream = (hipStream_t)stream_;
    unsigned char* wsb = (unsigned char*)workspace;
    const int k = d.k, n_pairs = N * k;

    // set_decoder_norm_to_unit_norm (train_sae.py:307) as part of the step: instead of a read-modify-write pass over
    // W_dec (151 MB), only the inverse row norms are computed (75 MB read); decode / dh use W_dec[j] * inv_norm[j] on the
    // fly and pv_sae_apply writes the normalised + updated rows -- W_dec holds exactly what the reference's holds at every
    // step boundary (un-normalised after the optimizer step, as there).
    PV_REQUIRE(!renorm || st->dec_inv_norm, "PV_SAE_RENORM_DECODER needs pv_sae_state.dec_inv_norm");
    const float* inv_norm = nullptr;
    plan->renorm_pending = renorm;
    if (renorm && !(flags & PV_SAE_INV_NORM_VALID)) {
        const int rn = sae_dec_inv_norm(d, st, stream);
        if (rn) return rn;
    }
    if (renorm) inv_norm = st->dec_inv_norm;
    PV_REQUIRE(!sae_is_gated(st), "pv_sae_step does not serve a gated state: pv_sae_gated_step");
    // transcoder (pv_sae_state.tc): the loss is taken against tc.target, the decoder adds b_dec_out and the skip term
    const bool tc = sae_is_tc(st);
    if (tc) {
        // (token-sharded form: batch_mean = the TARGET's global mean -- the x-side normaliser sae_prep derives from it is overwritten by
        // sae_tc_target_norm below, as in the dense step)
        const int rq = sae_tc_require(d, st, N);
        if (rq) return rq;
    }
    int rc = sae_encode_topk(plan, st, x, N, batch_mean, out->topk_idx, out->topk_val, true, wsb, ws, stream);
    if (rc) return rc;
    const float* skip = nullptr;
    if (tc) {
        rc = sae_tc_target_norm(d, st, batch_mean, N, wsb, ws, stream);
        if (rc) return rc;
        rc = sae_tc_skip_forward(d, st, x, N, &skip, stream);
        if (rc) return rc;
    }
    const float* y = tc ? st->tc.target : x;
    const float* bdo = tc ? (const float*)st->tc.b_dec_out : (const float*)st->b_dec;

    rc = sae_sparse_tail(plan, st, x, N, n_global, k, out->topk_idx, out->topk_val, out->sae_out, out->scalars, out->fire_count,
                         update_stats, sparse, inv_norm, sae_tail(wsb, ws, (size_t)n_pairs), wsb, ws, y, bdo, skip, tc, 0.0f, nullptr, nullptr,
                         stream, true,
                         (fused_sq && g_pv_tuning.sae_fold) ? out->scalars : (float*)nullptr);
    if (rc) return rc;
    if (fused_sq && !g_pv_tuning.sae_fold) {                          // (the A/B of the folds: the same sum as a launch of its own)
        hipLaunchKernelGGL(sqnorm_blocks_kernel, dim3(1), dim3(1024), 0, stream, (const float*)st->gb_dec, d.d_in,
                           (const float*)(wsb + ws.rowsq), d.d_sae, out->scalars);
        PV_LAUNCH_CHECK("sqnorm_blocks_kernel");
    }
    return PV_OK;
}
