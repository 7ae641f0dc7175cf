// Feature-parallel step (C ABI: pv_sae_tp_* in include/pv_native.h): this rank's engine covers a SHARD of the features; the
// top-k is taken over all ranks' candidates by the caller, the local candidates that did not make it arrive here with value 0 -- and a
// pair with value <= 0 is a hole everywhere (no decode contribution, no CSR entry, dh gated off), like the reference's ReLU behind
// its top-k.  pv_sae_step (sae.hip) cut at the reconstruction:
//   pv_sae_encode_topk (this rank's k candidates per token)  ->  [all-gather of candidate values, global top-k: caller]
//   pv_sae_tp_partial  (partial reconstruction of the kept pairs)  ->  [all-reduce of the partials: caller]
//   pv_sae_tp_finish   (LN-out, loss, dY, dh, CSR, sparse backward, statistics for the shard's features)
//   -> [gb_dec / clip norm / l0 all-reduces: caller] -> pv_sae_apply
#include "sae_bwd.hpp"

__global__ __launch_bounds__(256) void sae_recount_kernel(const int32_t* __restrict__ idx, const float* __restrict__ val,
                                                          uint32_t* __restrict__ cnt, uint32_t* __restrict__ wpos, int n_pairs) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pairs) return;
    wpos[i] = val[i] > 0.f ? atomicAdd(&cnt[idx[i]], 1u) : 0xffffffffu;
}

extern "C" int pv_sae_tp_partial(pv_sae_plan* plan, pv_sae_state* st, const int32_t* topk_idx, const float* topk_val, int32_t N,
                                 int32_t flags, float* partial, void* stream_) {
    PV_REQUIRE(!st || !sae_is_gated(st), "this entry point does not serve a gated state (pv_sae_state.gt)");
    PV_REQUIRE(!st || !sae_is_tc(st), "pv_sae_tp_partial: not available for a transcoder state (pv_sae_state.tc)");
    PV_REQUIRE(plan && st && topk_idx && topk_val && partial && st->W_dec, "null argument");
    const pv_sae_desc& d = plan->d;
    PV_REQUIRE(N >= 1 && N <= d.max_tokens, "n_tokens exceeds plan max_tokens");
    hipStream_t stream = (hipStream_t)stream_;
    const bool renorm = (flags & PV_SAE_RENORM_DECODER) != 0;
    PV_REQUIRE(!renorm || st->dec_inv_norm, "PV_SAE_RENORM_DECODER needs pv_sae_state.dec_inv_norm");
    plan->renorm_pending = renorm;
    plan->live_offs = nullptr;
    if (renorm && !(flags & PV_SAE_INV_NORM_VALID)) {
        const int rc = sae_dec_inv_norm(d, st, stream);
        if (rc) return rc;
    }
    SaeDecode dec;
    dec.mode = 1; dec.N = N; dec.d = d.d_in; dec.k = d.k;
    dec.W_dec = st->W_dec; dec.idx = topk_idx; dec.val = topk_val; dec.sae_out = partial;
    dec.inv_norm = renorm ? (const float*)st->dec_inv_norm : nullptr;
    return sae_decode(dec, stream);
}

// `workspace` must be the one the preceding pv_sae_encode_topk ran in, on the same x (it holds the LN statistics, the
// loss normaliser and sae_in); pre_sum [N, d_in] = the reconstruction summed over the ranks (without b_dec).  Gradients of
// the shard's rows are WRITTEN into st->g*; st->gb_dec receives colsum(dY) - W_enc[:, shard] gb_enc[shard]: the caller
// combines the ranks' encoder terms.  scalars[0..1] = loss (over the full batch, replicated), scalars[2] = this rank's
// kept pairs per token (the ranks' values add up to l0).
extern "C" int pv_sae_tp_finish(pv_sae_plan* plan, pv_sae_state* st, const float* x, const float* pre_sum, const int32_t* topk_idx,
                                const float* topk_val, int32_t N, int32_t n_global, int32_t flags, pv_sae_out* out,
                                void* workspace, size_t workspace_bytes, void* stream_) {
    PV_REQUIRE(!st || !sae_is_gated(st), "this entry point does not serve a gated state (pv_sae_state.gt)");
    PV_REQUIRE(!st || !sae_is_tc(st), "pv_sae_tp_finish: not available for a transcoder state (pv_sae_state.tc)");
    const int update_stats = (flags & PV_SAE_UPDATE_STATS) ? 1 : 0;
    PV_REQUIRE(plan && st && x && pre_sum && topk_idx && topk_val && out && workspace, "null argument");
    PV_REQUIRE(out->scalars, "pv_sae_out.scalars");
    PV_REQUIRE(st->W_dec && st->b_enc && st->b_dec && st->gW_enc && st->gW_dec && st->gb_enc && st->gb_dec, "state");
    PV_REQUIRE(st->W_encT, "the transposed encoder copy (pv_sae_state.W_encT) is required");
    PV_REQUIRE(!update_stats || (st->act_freq_scores && st->n_fwd_since_fired), "stats buffers");
    const pv_sae_desc& d = plan->d;
    PV_REQUIRE(N >= 1 && N <= d.max_tokens, "n_tokens exceeds plan max_tokens");
    PV_REQUIRE(n_global >= N, "n_global must be >= n_tokens");
    const SaeWs ws = sae_carve(d);
    PV_REQUIRE(workspace_bytes >= ws.total, "workspace too small");
    hipStream_t stream = (hipStream_t)stream_;
    unsigned char* wsb = (unsigned char*)workspace;
    const int k = d.k, n_pairs = N * k;
    plan->live_offs = nullptr;
    float* dY = (float*)(wsb + ws.dY);
    uint32_t* cnt = (uint32_t*)(wsb + ws.cnt);
    // the pairs that survived the global top-k: counts and within-list positions afresh
    PV_HIP_CHECK(hipMemsetAsync(cnt, 0, (size_t)d.d_sae * 4, stream));
    hipLaunchKernelGGL(sae_recount_kernel, dim3((n_pairs + 255) / 256), dim3(256), 0, stream, topk_idx, topk_val, cnt,
                       (uint32_t*)(wsb + ws.wpos), n_pairs);
    // sae_fold means here what it means for pv_sae_step (sae_sparse_tail): folded, the CSR scan is one more workgroup
    // of the decode launch, the loss rides in the post + fill launch and both list sorts are one launch -- 11 launches instead of 13
    const bool folded = g_pv_tuning.sae_fold != 0;
    SaeDecode dec;
    dec.mode = 2; dec.N = N; dec.d = d.d_in; dec.k = k;
    dec.x = x; dec.W_dec = st->W_dec; dec.b_dec = st->b_dec; dec.idx = topk_idx; dec.val = topk_val;
    dec.mu = (const float*)(wsb + ws.mu); dec.sd = (const float*)(wsb + ws.sd); dec.norm = (const float*)(wsb + ws.norm);
    dec.sae_out = out->sae_out; dec.dY = dY; dec.dh = (float*)(wsb + ws.dh); dec.loss_part = (float*)(wsb + ws.loss_part);
    dec.grad_scale = 2.0f / ((float)n_global * (float)d.d_in);
    dec.inv_norm = plan->renorm_pending ? (const float*)st->dec_inv_norm : nullptr;       // as pv_sae_tp_partial left it
    dec.pre_sum = pre_sum;
    if (folded) dec.scan = sae_scan_role(d, wsb, ws, cnt, out->scalars, N);
    int rc = sae_decode(dec, stream);
    if (rc) return rc;
    SaeBwd b;
    b.N = N; b.k = k; b.idx = topk_idx; b.val = topk_val; b.dY = dY; b.sae_in = (const float*)(wsb + ws.sae_in); b.scalars = out->scalars;
    b.tail = sae_tail(wsb, ws, (size_t)n_pairs);
    b.fire_count = out->fire_count; b.update_stats = update_stats;
    b.loss_part = (const float*)(wsb + ws.loss_part); b.loss_scale = 1.0f / ((float)n_global * (float)d.d_in);
    b.colsum_dY = true; b.folded = folded;
    rc = sae_csr_backward(plan, st, b, wsb, ws, stream);
    if (rc) return rc;
    // PV_SAE_TP_ENC_TERM_ONLY: every rank holds the same dY; only one of them contributes its column sum to the all-reduce
    return sae_gbdec(d, st, dY, N, wsb, ws, stream, (flags & PV_SAE_TP_ENC_TERM_ONLY) ? SAE_DY_NOWHERE : SAE_DY_TO_GB_DEC, true);
}

// ---- feature-parallel glue kernels: the global top-k over the ranks' candidates, and the ONE small all-reduce bucket ----
// gathered [W][2][N][k]: rank r's piece = its k candidate values per token (float bits, sorted or not) followed by their
// LOCAL feature indices (global index = r * shard + local).  A wave per token: lane s owns this rank's candidate s and
// counts the candidates of all ranks that come before it in the order (value desc, global feature index asc) -- torch.topk's
// order on the dense row, as the oracle -- out of an LDS copy of the token's W k candidates; rank < k = kept, otherwise
// the value becomes 0 (a hole).  Replaces two argsorts over [N, W k] and a scatter on the host side.
constexpr int MAXK = PV_SAE_MAXK;
__global__ __launch_bounds__(256) void sae_tp_merge_kernel(const int32_t* __restrict__ gathered, int W, int rank, int n_tok, int k,
                                                           int shard, float* __restrict__ val_kept) {
    __shared__ float sv[4][8 * MAXK];
    __shared__ int32_t sg[4][8 * MAXK];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int n = blockIdx.x * 4 + wv;
    if (n >= n_tok) return;                                    // (whole waves leave; no workgroup barrier below)
    const int64_t piece = 2 * (int64_t)n_tok * k;
    const int total = W * k;
    for (int c = lane; c < total; c += 64) {
        const int r = c / k, t = c - r * k;
        const int32_t* pr = gathered + r * piece + (int64_t)n * k + t;
        sv[wv][c] = __int_as_float(pr[0]);
        sg[wv][c] = r * shard + pr[(int64_t)n_tok * k];
    }
    __builtin_amdgcn_wave_barrier();                            // (a wave's LDS operations execute in order)
    if (lane < k) {
        const float v = sv[wv][rank * k + lane];
        const int32_t g = sg[wv][rank * k + lane];
        int before = 0;
        for (int c = 0; c < total; ++c) {
            const float vo = sv[wv][c];
            before += (vo > v) || (vo == v && sg[wv][c] < g);
        }
        val_kept[(int64_t)n * k + lane] = before < k ? v : 0.f;
    }
}

extern "C" int pv_sae_tp_merge(const int32_t* gathered, int32_t world, int32_t rank, int32_t N, int32_t k, int32_t shard,
                               float* val_kept, void* stream_) {
    PV_REQUIRE(gathered && val_kept, "null argument");
    PV_REQUIRE(world >= 1 && world <= 8 && rank >= 0 && rank < world, "world size must be in [1, 8]");
    PV_REQUIRE(k >= 1 && k <= MAXK && N >= 1 && shard >= k, "shape");
    hipLaunchKernelGGL(sae_tp_merge_kernel, dim3((N + 3) / 4), dim3(256), 0, (hipStream_t)stream_, gathered, world, rank, N, k, shard,
                       val_kept);
    PV_LAUNCH_CHECK("sae_tp_merge_kernel");
    return PV_OK;
}

// The bucket every rank all-reduces once per step: [gb_dec (d_in) | rows term of the clip norm | kept pairs per token | 2 pad |
// firing counts of ALL features (d_sae_total)].  pv_sae_tp_finish has already written this rank's gb_dec term and its
// shard's firing counts in place (the caller points st->gb_dec / out->fire_count into the bucket); pack adds the two
// scalars and zeroes the other ranks' firing counts.  After the all-reduce, unpack forms the clip norm of the GLOBAL
// gradient: the ranks' row terms + ||gb_dec||^2 of the summed gb_dec.
__global__ __launch_bounds__(1024) void sae_tp_bucket_pack_kernel(const float* __restrict__ rowsq, int d_shard, const float* __restrict__ scalars,
                                                                  float* __restrict__ bucket, int d_in, int j_lo, int d_total) {
    __shared__ float red[16];
    float s = 0.f;
    for (int j = threadIdx.x; j < d_shard; j += 1024) s += rowsq[j];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    float* fire = bucket + d_in + 4;
    for (int j = threadIdx.x; j < d_total; j += 1024)
        if (j < j_lo || j >= j_lo + d_shard) fire[j] = 0.f;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int w = 0; w < 16; ++w) t += red[w];
        bucket[d_in] = t;
        bucket[d_in + 1] = scalars[2];
        bucket[d_in + 2] = 0.f;
        bucket[d_in + 3] = 0.f;
    }
}
__global__ __launch_bounds__(1024) void sae_tp_bucket_unpack_kernel(const float* __restrict__ bucket, int d_in, float* __restrict__ scalars) {
    __shared__ float red[16];
    float s = 0.f;
    for (int i = threadIdx.x; i < d_in; i += 1024) s += bucket[i] * bucket[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int w = 0; w < 16; ++w) t += red[w];
        scalars[3] = bucket[d_in] + t;
        scalars[2] = bucket[d_in + 1];
    }
}

extern "C" int pv_sae_tp_bucket_pack(pv_sae_plan* plan, const void* workspace, const float* scalars, float* bucket, int32_t j_lo,
                                     int32_t d_sae_total, void* stream_) {
    PV_REQUIRE(plan && workspace && scalars && bucket, "null argument");
    const pv_sae_desc& d = plan->d;
    PV_REQUIRE(j_lo >= 0 && j_lo + d.d_sae <= d_sae_total, "shard range");
    const SaeWs ws = sae_carve(d);
    hipLaunchKernelGGL(sae_tp_bucket_pack_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream_,
                       (const float*)((const unsigned char*)workspace + ws.rowsq), d.d_sae, scalars, bucket, d.d_in, j_lo, d_sae_total);
    PV_LAUNCH_CHECK("sae_tp_bucket_pack_kernel");
    return PV_OK;
}
extern "C" int pv_sae_tp_bucket_unpack(pv_sae_plan* plan, const float* bucket, float* scalars, void* stream_) {
    PV_REQUIRE(plan && bucket && scalars, "null argument");
    hipLaunchKernelGGL(sae_tp_bucket_unpack_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream_, bucket, plan->d.d_in, scalars);
    PV_LAUNCH_CHECK("sae_tp_bucket_unpack_kernel");
    return PV_OK;
}
