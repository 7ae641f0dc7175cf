// Ghost gradients (SparseAutoencoder._compute_ghost_residual_loss, sae.py:151-179; gfx950): the part the dense ReLU + L1 step and the
// top-k pass share (ghost_residual, ghost_add_rows: sae_ghost.hpp), and the top-k pass itself (C ABI: pv_sae_topk_ghost).
#include "sae_ghost.hpp"

namespace {
// rows of W_dec of the dead features, compacted (zero rows up to the padded count)
__global__ __launch_bounds__(256) void ghost_gather_rows_kernel(const float* __restrict__ W_dec, const int32_t* __restrict__ dead_idx,
                                                                int n_dead, int n_pad, int d, float* __restrict__ out) {
    const int s = blockIdx.x;
    const float* src = s < n_dead ? W_dec + (int64_t)dead_idx[s] * d : nullptr;
    for (int c = threadIdx.x; c < d; c += 256) out[(int64_t)s * d + c] = src ? src[c] : 0.f;
}
// gW_dec[dead_idx[s]] += add[s]
__global__ __launch_bounds__(256) void ghost_scatter_add_rows_kernel(float* __restrict__ gW_dec, const int32_t* __restrict__ dead_idx,
                                                                     int n_dead, int d, const float* __restrict__ add) {
    const int s = blockIdx.x;
    if (s >= n_dead) return;
    float* dst = gW_dec + (int64_t)dead_idx[s] * d;
    for (int c = threadIdx.x; c < d; c += 256) dst[c] += add[(int64_t)s * d + c];
}
// A Transcoder's ghost term rescales by _compute_mse_loss(INPUT, sae_out) (transcoder.py:82-86, sae.py:144-149, 170-173): per token
// sum_i err_i^2 / ||x_n - mean_batch(x)||, err = sae_out - x.  One wave per token.
__global__ __launch_bounds__(256) void tc_ghost_mse_kernel(const float* __restrict__ x, const float* __restrict__ err,
                                                           const float* __restrict__ xmean, float* __restrict__ part, int n_tok, int d) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= n_tok) return;
    float c2 = 0.f, e2 = 0.f;
    for (int i = lane; i < d; i += 64) {
        const float c = x[(int64_t)n * d + i] - xmean[i], e = err[(int64_t)n * d + i];
        c2 += c * c; e2 += e * e;
    }
    c2 = wave_sum(c2); e2 = wave_sum(e2);
    if (lane == 0) part[n] = e2 / sqrtf(c2);
}

// One wave per token.  res = x - sae_out = -err; G0 = exp(hidden_pre[:, dead]) @ W_dec[dead]:
//   s = ||res|| / (1e-6 + 2 ||G0||)  (detached);  G = s G0;  den = || res - mean_batch(res) ||  (detached)
//   mg = (G - res)^2 / den;  r = mse_loss / (mg + 1e-6)  (detached);  ghost loss = mean(r mg)
//   d ghost / d G0 = s r 2 (G - res) / (den N d)
__global__ __launch_bounds__(256) void ghost_rows_kernel(const float* __restrict__ err, const float* __restrict__ G0,
                                                         const float* __restrict__ colmean_err, const float* __restrict__ mse_ptr,
                                                         float* __restrict__ dG0, float* __restrict__ part, int n_tok, int d,
                                                         float inv_count) {
    // colmean_err / mse_ptr / inv_count: over the GLOBAL batch (tokens sharded over ranks: pv_sae_ghost.err_colmean / mse_global /
    // n_global), this call's own batch otherwise
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= n_tok) return;
    const float* e = err + (int64_t)n * d;
    const float* g0 = G0 + (int64_t)n * d;
    float r2 = 0.f, g2 = 0.f, c2 = 0.f;
    for (int i = lane; i < d; i += 64) {
        const float res = -e[i], g = g0[i], rc = res + colmean_err[i];        // res - mean(res) = -(err - mean(err))
        r2 += res * res; g2 += g * g; c2 += rc * rc;
    }
    r2 = wave_sum(r2); g2 = wave_sum(g2); c2 = wave_sum(c2);
    const float s = sqrtf(r2) / (1e-6f + 2.0f * sqrtf(g2));
    const float den = sqrtf(c2);
    const float mse = *mse_ptr;
    float acc = 0.f;
    for (int i = lane; i < d; i += 64) {
        const float res = -e[i], diff = g0[i] * s - res;
        const float mg = diff * diff / den;
        const float r = mse / (mg + 1e-6f);
        acc += r * mg;
        dG0[(int64_t)n * d + i] = s * r * 2.0f * diff / den * inv_count;
    }
    acc = wave_sum(acc);
    if (lane == 0) part[n] = acc;
}

// out[s] = src[idx[s]] for s < n, pad_value up to n_pad
__global__ __launch_bounds__(256) void ghost_gather_vec_kernel(const float* __restrict__ src, const int32_t* __restrict__ idx, int n, int n_pad,
                                                               float pad_value, float* __restrict__ out) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s < n_pad) out[s] = s < n ? src[idx[s]] : pad_value;
}
// dst[idx[s]] += add[s]
__global__ __launch_bounds__(256) void ghost_scatter_add_vec_kernel(float* __restrict__ dst, const int32_t* __restrict__ idx, int n,
                                                                    const float* __restrict__ add) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s < n) dst[idx[s]] += add[s];
}
// err = sae_out - y
__global__ __launch_bounds__(256) void ghost_err_kernel(const float* __restrict__ sae_out, const float* __restrict__ y, float* __restrict__ err,
                                                        int64_t n4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const float4 a = reinterpret_cast<const float4*>(sae_out)[i], b = reinterpret_cast<const float4*>(y)[i];
    reinterpret_cast<float4*>(err)[i] = make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w);
}
// scalars[0] = mse + ghost residual loss (top-k: no L1 term), scalars[4] = 0
__global__ void topk_ghost_loss_kernel(float* __restrict__ scalars) {
    scalars[4] = 0.f;
    scalars[0] = scalars[1] + scalars[5];
}
}  // namespace

static GhostWs ghost_carve(const pv_sae_desc& d, int N, int n_dead) {
    GhostWs w;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (size_t)pv_align_up((int64_t)bytes, 256); return o; };
    w.n_pad = n_dead > 0 ? (n_dead + 7) / 8 * 8 : 0;
    const size_t P = w.n_pad, D = d.d_in, n = N;
    w.dead_act = take(n * P * 4);
    w.dhd = take(n * P * 4);
    w.wdd = take(P * D * 4);
    w.tmpw = take(P * D * 4);
    w.g0 = take(n * D * 4);
    w.dg0 = take(n * D * 4);
    w.err = take(n * D * 4);
    w.colmean = take(D * 4);
    w.part = take(n * 4);
    w.colpart = take((n / 16 + 2) * D * 4);
    w.vec_a = take((P + 8) * 4);                       // pv_sae_topk_ghost: b_enc of the dead features / column sums over them
    w.vec_b = take((P + 8) * 4);
    w.colpart_p = take((n / 16 + 2) * (P + 8) * 4);
    w.total = off + 256;
    return w;
}

extern "C" size_t pv_sae_ghost_workspace_bytes(const pv_sae_plan* plan, int32_t n_tokens, int32_t n_dead) {
    if (!plan || n_tokens < 1 || n_dead < 0) return 0;
    return ghost_carve(plan->d, n_tokens, n_dead).total;
}

int ghost_require(const pv_sae_desc& d, int N, const pv_sae_ghost* ghost, GhostWs* gw) {
    const int nd = ghost->n_dead;
    PV_REQUIRE(nd >= 0 && nd <= d.d_sae && ghost->workspace && (nd == 0 || (ghost->dead_idx && ghost->dead_slot)), "pv_sae_ghost");
    *gw = ghost_carve(d, N, nd);
    PV_REQUIRE(ghost->workspace_bytes >= gw->total && ((uintptr_t)ghost->workspace & 255) == 0, "ghost workspace too small / misaligned");
    return PV_OK;
}

int ghost_residual(const pv_sae_desc& d, const pv_sae_state* st, const float* x, int N, const pv_sae_ghost* ghost, const GhostWs& gw,
                   float* scalars, float inv_cnt, hipStream_t stream) {
    unsigned char* gwb = (unsigned char*)ghost->workspace;
    const int nd = ghost->n_dead, D = d.d_in, P = gw.n_pad;
    const bool tc = sae_is_tc(st);
    float *g0 = (float*)(gwb + gw.g0), *dg0 = (float*)(gwb + gw.dg0), *act = (float*)(gwb + gw.dead_act), *wdd = (float*)(gwb + gw.wdd);
    float *cm = (float*)(gwb + gw.colmean), *colpart = (float*)(gwb + gw.colpart), *part = (float*)(gwb + gw.part);
    const float* err = (const float*)(gwb + gw.err);
    int rc = PV_OK;
    if (nd > 0) {
        hipLaunchKernelGGL(ghost_gather_rows_kernel, dim3(P), dim3(256), 0, stream, (const float*)st->W_dec, ghost->dead_idx, nd, P, D, wdd);
        DenseGemm gg = {};
        gg.A = act; gg.lda = P; gg.B = wdd; gg.ldb = D; gg.M = N; gg.N = D; gg.K = P; gg.k_chunk = P;
        gg.out = g0; gg.ldo = D;
        rc = launch_dense_gemm<false, true, DG_EPI_STORE>(gg, 1, stream);
        if (rc) return rc;
    } else {
        PV_HIP_CHECK(hipMemsetAsync(g0, 0, (size_t)N * D * 4, stream));
    }
    if (tc) {
        // a transcoder's ghost term rescales by _compute_mse_loss(INPUT, sae_out) (-> scalars[7]; err = sae_out - x), not by the step's mse
        // against the target; cm / colpart / part are re-used below for the residual's own column mean
        rc = sae_colsum(x, N, D, cm, 1.0f / (float)N, colpart, stream);
        if (rc) return rc;
        hipLaunchKernelGGL(tc_ghost_mse_kernel, dim3((N + 3) / 4), dim3(256), 0, stream, x, err, (const float*)cm, part, N, D);
        PV_LAUNCH_CHECK("tc_ghost_mse_kernel");
        sae_reduce_sum(part, scalars, N, 1.0f / ((float)N * (float)D), 7, -1, stream);
    }
    const float* colmean = ghost->err_colmean;
    if (!colmean) {
        rc = sae_colsum(err, N, D, cm, 1.0f / (float)N, colpart, stream);
        if (rc) return rc;
        colmean = cm;
    }
    hipLaunchKernelGGL(ghost_rows_kernel, dim3((N + 3) / 4), dim3(256), 0, stream, err, (const float*)g0, colmean,
                       ghost->mse_global ? ghost->mse_global : (const float*)(scalars + (tc ? 7 : 1)), dg0, part, N, D, inv_cnt);
    PV_LAUNCH_CHECK("ghost_rows_kernel");
    sae_reduce_sum(part, scalars, N, inv_cnt, 5, -1, stream);
    if (nd == 0) return PV_OK;
    DenseGemm gb = {};
    gb.A = dg0; gb.lda = D; gb.B = wdd; gb.ldb = D; gb.M = N; gb.N = P; gb.K = D; gb.k_chunk = D;
    gb.out = (float*)(gwb + gw.dhd); gb.ldo = P; gb.mul = act;
    return launch_dense_gemm<false, false, DG_EPI_MUL>(gb, 1, stream);
}

int ghost_add_rows(const float* A, int64_t lda, const float* B, int M, int K, float* dst, const pv_sae_ghost* ghost, const GhostWs& gw, int d_in,
                   hipStream_t stream) {
    float* tmpw = (float*)((unsigned char*)ghost->workspace + gw.tmpw);
    DenseGemm gt = {};
    gt.A = A; gt.lda = lda; gt.B = B; gt.ldb = d_in; gt.M = M; gt.N = d_in; gt.K = K; gt.k_chunk = K; gt.out = tmpw; gt.ldo = d_in;
    const int rc = launch_dense_gemm<true, true, DG_EPI_STORE>(gt, 1, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(ghost_scatter_add_rows_kernel, dim3(ghost->n_dead), dim3(256), 0, stream, dst, ghost->dead_idx, ghost->n_dead, d_in,
                       (const float*)tmpw);
    PV_LAUNCH_CHECK("ghost_scatter_add_rows_kernel");
    return PV_OK;
}

// Ghost gradients on a TOP-K SAE (use_ghost_grads with activation_fn_str = "topk": SparseAutoencoder._compute_ghost_residual_loss,
// sae.py:151-179, behind TopK :795-810; the dead mask of train_sae.py:330-332).  Runs AFTER pv_sae_step on the same batch (complete
// gradient buffers: no PV_SAE_SPARSE_GRADS; the decoder renormalised in place beforehand: pv_sae_renorm_decoder, no
// PV_SAE_RENORM_DECODER) and adds what the ghost term contributes: exp(hidden_pre) of the dead features is ONE small GEMM
// (sae_in against the gathered rows of W_encT, exp in its epilogue -- the k-sparse encoder never materialises hidden_pre), the
// ghost reconstruction, its loss (scalars[5]; scalars[0] = mse + ghost) and gradient as in pv_sae_dense_step, and the gradient
// reaches the dead features' rows of gW_dec, gW_enc^T, gb_enc (row scatter-adds) and gb_dec (recomputed).  The per-feature
// norm terms of the step are stale afterwards: follow with pv_sae_grad_sqnorm over the whole flat buffer, then pv_sae_apply.
// out->sae_out must be the reconstruction pv_sae_step wrote; ghost as for pv_sae_dense_step.  Single process, no transcoder.
extern "C" int pv_sae_topk_ghost(pv_sae_plan* plan, pv_sae_state* st, const float* x, int32_t N, const pv_sae_ghost* ghost, pv_sae_out* out,
                                 void* workspace, size_t workspace_bytes, void* stream_) {
    PV_REQUIRE(plan && st && x && ghost && out && workspace, "null argument");
    PV_REQUIRE(out->sae_out && out->scalars, "pv_sae_out: sae_out (as pv_sae_step wrote it) and scalars are required");
    PV_REQUIRE(st->W_dec && st->W_encT && st->b_enc && st->gW_enc && st->gW_dec && st->gb_enc && st->gb_dec, "state");
    PV_REQUIRE(!sae_is_gated(st), "top-k ghost gradients: not for a gated SAE");
    const bool tc = sae_is_tc(st);
    // a Transcoder (round 6): x = the INPUT activation -- the ghost residual is input - sae_out (transcoder.py:82-86); equal widths, one process
    PV_REQUIRE(!tc || (st->tc.d_in_true <= 0 && st->tc.d_out_true <= 0 && ghost->n_global <= N && !ghost->mse_global),
               "transcoder + ghost gradients: d_out == d_in and the whole batch in one process");
    PV_REQUIRE(!plan->renorm_pending, "top-k ghost gradients need the decoder renormalised IN PLACE before the step (pv_sae_renorm_decoder), "
                                      "not deferred (PV_SAE_RENORM_DECODER)");
    const pv_sae_desc& d = plan->d;
    PV_REQUIRE(N >= 1 && N <= d.max_tokens, "n_tokens exceeds plan max_tokens");
    PV_REQUIRE(d.d_in % 8 == 0, "d_in must be a multiple of 8");
    const int nd = ghost->n_dead, D = d.d_in;
    GhostWs gw;
    int rc = ghost_require(d, N, ghost, &gw);
    if (rc) return rc;
    const int ng = ghost->n_global > 0 ? ghost->n_global : N;
    PV_REQUIRE(ng >= N && (ng == N || (ghost->err_colmean && ghost->mse_global)),
               "pv_sae_ghost.n_global > n_tokens needs err_colmean and mse_global (the global batch's)");
    const SaeWs ws = sae_carve(d);
    PV_REQUIRE(workspace_bytes >= ws.total && ((uintptr_t)workspace & 255) == 0, "workspace too small / misaligned");
    hipStream_t stream = (hipStream_t)stream_;
    unsigned char* wsb = (unsigned char*)workspace;
    unsigned char* gwb = (unsigned char*)ghost->workspace;
    const float* sae_in = (const float*)(wsb + ws.sae_in);
    const float* dY = (const float*)(wsb + ws.dY);
    float* err = (float*)(gwb + gw.err);
    float* act = (float*)(gwb + gw.dead_act);
    float* tmpw = (float*)(gwb + gw.tmpw);
    float* dhd = (float*)(gwb + gw.dhd);
    const int P = gw.n_pad;
    hipLaunchKernelGGL(ghost_err_kernel, dim3((unsigned)(((int64_t)N * D / 4 + 255) / 256)), dim3(256), 0, stream,
                       (const float*)out->sae_out, x, err, (int64_t)N * D / 4);
    if (nd > 0) {
        // E = exp(sae_in @ W_enc[:, dead] + b_enc[dead]): the rows of W_encT of the dead features, gathered (tmpw holds them until it is
        // needed for the gradients); padding columns get a bias of -1e30 (E = 0 there)
        hipLaunchKernelGGL(ghost_gather_rows_kernel, dim3(P), dim3(256), 0, stream, (const float*)st->W_encT, ghost->dead_idx, nd, P, D, tmpw);
        hipLaunchKernelGGL(ghost_gather_vec_kernel, dim3((P + 255) / 256), dim3(256), 0, stream, (const float*)st->b_enc, ghost->dead_idx, nd, P,
                           -1e30f, (float*)(gwb + gw.vec_a));
        DenseGemm ge = {};
        ge.A = sae_in; ge.lda = D; ge.B = tmpw; ge.ldb = D; ge.M = N; ge.N = P; ge.K = D; ge.k_chunk = D;
        ge.out = act; ge.ldo = P; ge.bias = (const float*)(gwb + gw.vec_a);
        rc = launch_dense_gemm<false, false, DG_EPI_EXPB>(ge, 1, stream);
        if (rc) return rc;
    }
    rc = ghost_residual(d, st, x, N, ghost, gw, out->scalars, 1.0f / ((float)ng * (float)D), stream);
    if (rc) return rc;
    hipLaunchKernelGGL(topk_ghost_loss_kernel, dim3(1), dim3(1), 0, stream, out->scalars);
    if (nd > 0) {
        // gW_dec[dead] += E^T @ dG0;  gW_enc^T[dead] += dHd^T @ sae_in
        rc = ghost_add_rows(act, P, (const float*)(gwb + gw.dg0), P, N, st->gW_dec, ghost, gw, D, stream);
        if (rc) return rc;
        rc = ghost_add_rows(dhd, P, sae_in, P, N, st->gW_enc, ghost, gw, D, stream);
        if (rc) return rc;
        // gb_enc[dead] += colsum(dHd); gb_dec = colsum(dY) - W_enc gb_enc again
        rc = sae_colsum(dhd, N, P, (float*)(gwb + gw.vec_b), 1.0f, (float*)(gwb + gw.colpart_p), stream);
        if (rc) return rc;
        hipLaunchKernelGGL(ghost_scatter_add_vec_kernel, dim3((nd + 255) / 256), dim3(256), 0, stream, st->gb_enc, ghost->dead_idx, nd,
                           (const float*)(gwb + gw.vec_b));
        PV_LAUNCH_CHECK("ghost scatter kernels");
        rc = sae_gbdec(d, st, dY, N, wsb, ws, stream, tc ? SAE_DY_TO_GB_DEC_OUT : SAE_DY_TO_GB_DEC);
        if (rc) return rc;
    }
    plan->live_offs = nullptr;
    return PV_OK;
}
