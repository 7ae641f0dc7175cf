// Dense SAE train step for the activations that are NOT k-sparse: ReLU + L1 (gfx950; C ABI: pv_sae_dense_step).
//
// Reference semantics: StandardSparseAutoencoder.forward with activation_fn_str = "relu" (/root/reference/src/vit_prisma/
// sae/sae.py:557-645: encode :557-581, decode :583-595, mse :144-149, L1 sparsity :617-626 with lp_norm = 1) and the body of
// VisionSAETrainer.train_step between zero_grad and clip (sae/train_sae.py:328-392).  Every published CLIP SAE of the
// reference is of this kind (docs/sae_table.md:9-36).  A token keeps hundreds to thousands of its d_sae features, so the
// k-sparse machinery of sae.hip does not apply: the step is five dense GEMMs of 2 N d_in d_sae FLOP each.  They run on the
// EXACT fp32 matrix instruction (v_mfma_f32_32x32x2_f32 == an fmaf chain per output: no reduced-precision operand, results
// equal to the reference's fp32 matmuls up to summation order, measured <= 2e-6 relative), and everything elementwise rides
// in their epilogues -- no [N, d_sae] tensor is read or written except f itself (once) and dH over it (in place):
//
//   prep      (sae.hip)  LN-in, sae_in = x_hat - b_dec, loss normaliser
//   G1  f  = relu(sae_in W_enc + b_enc)  (W_enc^T read)  epilogue: bias, ReLU, store f; per-64-row column counts of f > 0
//                                                        (firing statistics, l0) and per-wave sums of f (the L1 term)
//   G2  pre = f W_dec  (split-K: [tokens x d_in] is only 192 tiles)   -> partial sums
//   finish    sae_out = (pre + b_dec) std + mu, err, mse partials, dY                  (one wave per token)
//   G4  gW_dec   = f^T dY                               straight into the flat gradient buffer
//   G3  dH = (dY W_dec^T + l1 / N) [f > 0]              epilogue: gate by the stored f, written OVER f; per-64-row column sums
//                                                        (gb_enc)
//   G5  gW_enc^T = dH^T sae_in                          straight into the flat gradient buffer (transposed encoder layout)
//   gb_dec = colsum(dY) - W_enc gb_enc   (sae.hip)
// then pv_sae_grad_sqnorm / pv_sae_apply (clip -> project -> Adam) as for the top-k step.
//
// Operand layouts: the fp32 matrix instruction takes ONE float per lane and operand, so a matrix can be fed from either of
// its two row-major layouts without a transposed copy -- K-contiguous rows ([rows][K]: one 16-byte LDS read = four k-steps) or
// row-contiguous k-slices ([K][rows]: four 4-byte LDS reads, lanes on consecutive rows).  f^T, dH^T, dY and sae_in of G4 / G5
// are therefore the buffers as they lie, read "the other way" (the kernel: sae_dense_gemm.hip; ghost gradients: sae_ghost.hip).
#include "sae_bwd.hpp"
#include "sae_ghost.hpp"
#include <cstring>

namespace {
// decoder output from the split-K partial sums: LN-out (sae.py:89-90), mse partial (sae.py:144-149), dY.  One wave per token.
__global__ __launch_bounds__(256) void dense_finish_kernel(const float* __restrict__ x, const float* __restrict__ kpart, int splits,
                                                           int64_t zstride, const float* __restrict__ b_dec, const float* __restrict__ mu,
                                                           const float* __restrict__ sd, const float* __restrict__ norm,
                                                           float* __restrict__ sae_out, float* __restrict__ dY,
                                                           float* __restrict__ loss_partial, int n_tok, int d, float grad_scale,
                                                           float* __restrict__ err_out, const float* __restrict__ addend,
                                                           const uint32_t* __restrict__ gate = nullptr,
                                                           const float* __restrict__ ghost_x = nullptr, uint32_t* __restrict__ amax = nullptr) {
    // amax (or NULL): partial maxima of |dY| (DG_AMAX_SLOTS words, see DenseGemm.a_max)
    // transcoder (pv_sae_state.tc): x = the TARGET, b_dec = b_dec_out, addend = the skip term or nullptr; ghost_x (a transcoder with
    // ghost gradients): the INPUT activation -- err_out is then sae_out - input, what the ghost term is computed on (transcoder.py:82-86)
    if (gate && *gate != 1u) return;
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= n_tok) return;
    const float m = mu[n], sdv = sd[n], nf = norm[n];
    float lsum = 0.f, gmax = 0.f;
    for (int c = 4 * lane; c < d; c += 256) {
        float4 a = *reinterpret_cast<const float4*>(kpart + (int64_t)n * d + c);
        for (int z = 1; z < splits; ++z) {
            const float4 t = *reinterpret_cast<const float4*>(kpart + z * zstride + (int64_t)n * d + c);
            a.x += t.x; a.y += t.y; a.z += t.z; a.w += t.w;
        }
        if (addend) {
            const float4 t = *reinterpret_cast<const float4*>(addend + (int64_t)n * d + c);
            a.x += t.x; a.y += t.y; a.z += t.z; a.w += t.w;
        }
        const float4 bd = *reinterpret_cast<const float4*>(b_dec + c);
        const float4 xv = *reinterpret_cast<const float4*>(x + (int64_t)n * d + c);
        float4 o, e, g;
        o.x = (a.x + bd.x) * sdv + m; o.y = (a.y + bd.y) * sdv + m; o.z = (a.z + bd.z) * sdv + m; o.w = (a.w + bd.w) * sdv + m;
        e.x = o.x - xv.x; e.y = o.y - xv.y; e.z = o.z - xv.z; e.w = o.w - xv.w;
        if (sae_out) *reinterpret_cast<float4*>(sae_out + (int64_t)n * d + c) = o;
        if (err_out) {
            float4 eg = e;
            if (ghost_x) {
                const float4 gx = *reinterpret_cast<const float4*>(ghost_x + (int64_t)n * d + c);
                eg.x = o.x - gx.x; eg.y = o.y - gx.y; eg.z = o.z - gx.z; eg.w = o.w - gx.w;
            }
            *reinterpret_cast<float4*>(err_out + (int64_t)n * d + c) = eg;
        }
        lsum += (e.x * e.x) / nf + (e.y * e.y) / nf + (e.z * e.z) / nf + (e.w * e.w) / nf;
        g.x = grad_scale * e.x / nf * sdv; g.y = grad_scale * e.y / nf * sdv;
        g.z = grad_scale * e.z / nf * sdv; g.w = grad_scale * e.w / nf * sdv;
        *reinterpret_cast<float4*>(dY + (int64_t)n * d + c) = g;
        gmax = fmaxf(fmaxf(gmax, fmaxf(fabsf(g.x), fabsf(g.y))), fmaxf(fabsf(g.z), fabsf(g.w)));
    }
    lsum = wave_sum(lsum);
    if (lane == 0) loss_partial[n] = lsum;
    if (amax) {
        gmax = wave_max(gmax);
        if (lane == 0) atomicMax(amax + (n & (DG_AMAX_SLOTS - 1)), __float_as_uint(gmax));
    }
}

// lp_norm > 1 (sae.py:617): per token S = sum_j f^p from the ENC epilogue's partials -> ||f_n||_p = S^(1/p) (the loss term) and
// l1 / N_global * S^(1/p - 1), the per-token factor of d ||f_n||_p / d f_j = S^(1/p - 1) f_j^(p - 1).  One wave per token, fixed order.
__global__ __launch_bounds__(256) void dense_lp_finish_kernel(const float* __restrict__ part, int ncb, float p, float l1_over_n,
                                                              float* __restrict__ lp_tok, float* __restrict__ lp_loss, int n_tok,
                                                              const uint32_t* __restrict__ gate) {
    if (gate && *gate != 1u) return;
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= n_tok) return;
    float s = 0.f;
    for (int c = lane; c < ncb; c += 64) s += part[(int64_t)n * ncb + c];
    s = wave_sum(s);
    if (lane == 0) {
        lp_loss[n] = s > 0.f ? powf(s, 1.f / p) : 0.f;
        lp_tok[n] = s > 0.f ? l1_over_n * powf(s, 1.f / p - 1.f) : 0.f;
    }
}

// scalars[0] = mse + l1 (+ ghost) (sae.py:628), one thread
__global__ void dense_loss_kernel(float* __restrict__ scalars, int ghost, const uint32_t* __restrict__ gate = nullptr, uint32_t want = 1u) {
    if (gate && *gate != want) return;
    if (!ghost) scalars[5] = 0.f;
    scalars[0] = scalars[1] + scalars[4] + scalars[5];
}

// out[i] = sum_z part[z * zstride + i] (fixed order): the split-K partials of gW_skip
__global__ __launch_bounds__(256) void dense_sumz_kernel(const float* __restrict__ part, int splits, int64_t zstride, int64_t n,
                                                         float* __restrict__ out) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    float4 a = *reinterpret_cast<const float4*>(part + i);
    for (int z = 1; z < splits; ++z) {
        const float4 t = *reinterpret_cast<const float4*>(part + z * zstride + i);
        a.x += t.x; a.y += t.y; a.z += t.z; a.w += t.w;
    }
    *reinterpret_cast<float4*>(out + i) = a;
}
}  // namespace

// ---- transcoder skip connection (sae/transcoder.py:73-76): two more GEMMs on the same kernel ---------------------------------
int sae_tc_skip_forward(const pv_sae_desc& d, const pv_sae_state* st, const float* x, int N, const float** skip, hipStream_t stream) {
    *skip = nullptr;
    if (!st->tc.W_skip) return PV_OK;
    const int D = d.d_in;
    float* buf = (float*)st->tc.scratch;                    // [N][D]
    DenseGemm g = {};
    g.A = x; g.lda = D; g.B = st->tc.W_skip; g.ldb = D; g.M = N; g.N = D; g.K = D; g.k_chunk = D;      // x @ W_skip^T: B as [N][K]
    g.out = buf; g.ldo = D;
    const int rc = launch_dense_gemm<false, false, DG_EPI_STORE>(g, 1, stream);
    if (rc) return rc;
    *skip = buf;
    return PV_OK;
}

int sae_tc_skip_backward(const pv_sae_desc& d, const pv_sae_state* st, const float* x, const float* dY, int N, hipStream_t stream) {
    if (!st->tc.W_skip) return PV_OK;
    const int D = d.d_in;
    float* part = (float*)st->tc.scratch + (size_t)N * D;   // [S][D][D]
    // gW_skip[o][i] = sum_n dY[n][o] x[n][i]: both operands row-major over the tokens, K = N split over the workgroups
    int S = (N + DG_KSLAB - 1) / DG_KSLAB;
    if (S > PV_SAE_SKIP_SPLITK) S = PV_SAE_SKIP_SPLITK;
    DenseGemm g = {};
    g.A = dY; g.lda = D; g.B = x; g.ldb = D; g.M = D; g.N = D; g.K = N;
    g.k_chunk = ((N + S - 1) / S + DG_KSLAB - 1) / DG_KSLAB * DG_KSLAB;
    g.out = part; g.ldo = D; g.out_zstride = (int64_t)D * D;
    const int rc = launch_dense_gemm<true, true, DG_EPI_STORE>(g, S, stream);
    if (rc) return rc;
    const int64_t n = (int64_t)D * D;
    hipLaunchKernelGGL(dense_sumz_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, stream, (const float*)part, S, n, n,
                       st->tc.gW_skip);
    PV_LAUNCH_CHECK("dense_sumz_kernel");
    return PV_OK;
}

namespace {
// validation shared by pv_sae_dense_step and pv_sae_relu_step
int dense_require(pv_sae_plan* plan, pv_sae_state* st, const float* x, int32_t N, int32_t n_global, int update_stats, pv_sae_out* out,
                  void* workspace, size_t workspace_bytes) {
    PV_REQUIRE(plan && st && x && out && workspace, "null argument");
    PV_REQUIRE(out->scalars, "pv_sae_out.scalars");
    PV_REQUIRE(st->W_dec && st->b_enc && st->b_dec && st->gW_enc && st->gW_dec && st->gb_enc && st->gb_dec, "state");
    PV_REQUIRE(st->W_encT, "the transposed encoder copy (pv_sae_state.W_encT) is required");
    PV_REQUIRE(!update_stats || (st->act_freq_scores && st->n_fwd_since_fired), "stats buffers");
    const pv_sae_desc& d = plan->d;
    PV_REQUIRE(N >= 1 && N <= d.max_tokens, "n_tokens exceeds plan max_tokens");
    PV_REQUIRE(n_global >= N, "n_global must be >= n_tokens");
    PV_REQUIRE(d.d_in % 8 == 0 && d.d_sae % 8 == 0, "the dense step needs d_in and d_sae to be multiples of 8");
    PV_REQUIRE(workspace_bytes >= sae_carve(d).total, "workspace too small");
    PV_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace alignment");
    return sae_is_tc(st) ? sae_tc_require(d, st, N) : PV_OK;
}

// renorm (flags), LN-in / sae_in / loss normaliser, the transcoder's target normaliser and skip term: what both forms of the
// ReLU + L1 step start from
int dense_prepare(pv_sae_plan* plan, pv_sae_state* st, const float* x, int N, const float* batch_mean, int flags, bool want_filter_inputs,
                  unsigned char* wsb, const SaeWs& ws, const float** skip, void* stream_) {
    const pv_sae_desc& d = plan->d;
    hipStream_t stream = (hipStream_t)stream_;
    plan->live_offs = nullptr;
    plan->renorm_pending = false;
    // set_decoder_norm_to_unit_norm (train_sae.py:307): the dense GEMMs read W_dec as it lies, so the rows are rewritten here
    if (flags & PV_SAE_RENORM_DECODER) {
        int rc = pv_sae_renorm_decoder(plan, st, stream_);
        if (rc) return rc;
    }
    int rc = sae_prep(d, x, (const float*)st->b_dec, batch_mean, N, want_filter_inputs, wsb, ws, stream, sae_in_width(d, st));
    if (rc) return rc;
    *skip = nullptr;
    if (sae_is_tc(st)) {
        rc = sae_tc_target_norm(d, st, batch_mean, N, wsb, ws, stream);
        if (rc) return rc;
        rc = sae_tc_skip_forward(d, st, x, N, skip, stream);
        if (rc) return rc;
    }
    return PV_OK;
}

// The five GEMMs + their small kernels (see the file header); `gate` as in DenseGemm.
int dense_step_body(pv_sae_plan* plan, pv_sae_state* st, const float* x, int32_t N, int32_t n_global, int update_stats,
                    float l1_coefficient, const pv_sae_ghost* ghost, const GhostWs& gw, pv_sae_out* out, unsigned char* wsb,
                    const SaeWs& ws, const float* skip, const uint32_t* gate, hipStream_t stream) {
    const pv_sae_desc& d = plan->d;
    const int F = d.d_sae, D = d.d_in;
    const bool tc = sae_is_tc(st);
    unsigned char* gwb = ghost ? (unsigned char*)ghost->workspace : nullptr;
    const int nd = ghost ? ghost->n_dead : 0;
    int rc = PV_OK;
    float* f = (float*)(wsb + ws.hidden);                  // [N][F]: f, later dH
    float* sae_in = (float*)(wsb + ws.sae_in);
    float* dY = (float*)(wsb + ws.dY);
    float* colpart = (float*)(wsb + ws.dense_colpart);
    float* rowpart = (float*)(wsb + ws.dense_rowpart);
    float* kpart = (float*)(wsb + ws.dense_kpart);
    const int rblk = (N + 63) / 64, cblk = (F + 63) / 64;
    const int nb_f = (F + 255) / 256;
    float* blk_tot = (float*)(wsb + ws.sqpart);            // 1024 floats of scratch (nb_f <= 256)
    // operand maxima of the split-fp16 GEMMs (see dense_gemm_kernel): sae_in, W_enc^T, f, W_dec, dY, dH.  The three that exist before
    // the first GEMM are taken here, dY behind the finish kernel, f and dH by the epilogues that write them.
    const DenseAmax am = {(uint32_t*)(wsb + ws.dense_amax)};
    enum { AM_X = DG_AM_X, AM_WENC = DG_AM_WENC, AM_F = 2, AM_WDEC = DG_AM_WDEC, AM_DY = 4, AM_DH = 5 };
    const bool split = dense_split_ok(d, N);
    const bool lp_on = d.lp_norm != 0.f && d.lp_norm != 1.f;      // the sparsity term is ||f_n||_p, p > 1 (sae.py:617)
    if (split) {
        rc = dense_absmax3(d, st, sae_in, N, am.base, gate, stream);
        if (rc) return rc;
    }
    {
        ProfScope prof(PV_PROF_SAE_ENC, stream, 2.0 * N * (double)D * F, ((double)N * D + (double)D * F + (double)N * F) * 4.0);
        // G1: f = relu(sae_in @ W_enc + b_enc)
        DenseGemm g = {};
        // (W_enc is read as its transposed fp32 master W_encT [F][D] -- the copy Adam runs in, always current; the parameter's
        // own layout may be materialised lazily)
        g.A = sae_in; g.lda = D; g.B = st->W_encT; g.ldb = D; g.M = N; g.N = F; g.K = D; g.k_chunk = D;
        g.out = f; g.ldo = F; g.bias = st->b_enc; g.colpart = colpart; g.rowpart = rowpart; g.gate = gate;
        if (split) { g.a_max = am(AM_X); g.b_max = am(AM_WENC); g.amax_out = am(AM_F); }
        g.act = d.activation; g.lp = d.lp_norm;
        if (lp_on) g.lp_part = (float*)(wsb + ws.dense_lp_part);
        if (nd > 0) {
            PV_HIP_CHECK(hipMemsetAsync(gwb + gw.dead_act, 0, (size_t)N * gw.n_pad * 4, stream));       // (padding columns stay zero)
            g.dead_slot = ghost->dead_slot; g.dead_act = (float*)(gwb + gw.dead_act); g.ldd = gw.n_pad;
        }
        rc = sae_plain_relu(d) ? launch_dense_gemm<false, false, DG_EPI_ENC>(g, 1, stream) : launch_dense_gemm<false, false, DG_EPI_ENC_T>(g, 1, stream);
        if (rc) return rc;
        // firing counts, statistics, l0, l1
        rc = dense_colreduce(colpart, rblk, F, out->fire_count ? out->fire_count : (float*)(wsb + ws.rowsq), st->act_freq_scores,
                             st->n_fwd_since_fired, update_stats, blk_tot, gate, stream);
        if (rc) return rc;
        sae_reduce_sum(blk_tot, out->scalars, nb_f, 1.0f / (float)N, 2, -1, stream, gate, 1u);                       // l0 (train_sae.py:364)
        if (lp_on) {
            // l1_loss = l1 * mean_n ||f_n||_p (sae.py:617-626 with lp_norm = p)
            hipLaunchKernelGGL(dense_lp_finish_kernel, dim3((N + 3) / 4), dim3(256), 0, stream, (const float*)(wsb + ws.dense_lp_part), cblk,
                               d.lp_norm, l1_coefficient / (float)n_global, (float*)(wsb + ws.dense_lp_tok), (float*)(wsb + ws.dense_lp_loss),
                               N, gate);
            PV_LAUNCH_CHECK("dense_lp_finish_kernel");
            sae_reduce_sum((const float*)(wsb + ws.dense_lp_loss), out->scalars, N, l1_coefficient / (float)n_global, 4, -1, stream, gate, 1u);
        } else {
            sae_reduce_sum(rowpart, out->scalars, rblk * cblk, l1_coefficient / (float)n_global, 4, -1, stream, gate, 1u);  // l1_loss (sae.py:617-626)
        }
    }
    {
        ProfScope prof(PV_PROF_SAE_BWD, stream, 8.0 * N * (double)D * F, 0.0);
        // G2: pre = f @ W_dec, split over K
        const int S = PV_SAE_DENSE_SPLITK;
        DenseGemm g = {};
        g.A = f; g.lda = F; g.B = st->W_dec; g.ldb = D; g.M = N; g.N = D; g.K = F;
        g.k_chunk = ((F + S - 1) / S + DG_KSLAB - 1) / DG_KSLAB * DG_KSLAB;
        g.out = kpart; g.ldo = D; g.out_zstride = (int64_t)N * D; g.gate = gate;
        if (split) { g.a_max = am(AM_F); g.b_max = am(AM_WDEC); }
        rc = launch_dense_gemm<false, true, DG_EPI_STORE>(g, S, stream);
        if (rc) return rc;
        const float grad_scale = 2.0f / ((float)n_global * (float)sae_loss_width(d, st));
        hipLaunchKernelGGL(dense_finish_kernel, dim3((N + 3) / 4), dim3(256), 0, stream, tc ? st->tc.target : x, (const float*)kpart, S,
                           (int64_t)N * D, tc ? (const float*)st->tc.b_dec_out : (const float*)st->b_dec, (const float*)(wsb + ws.mu),
                           (const float*)(wsb + ws.sd), (const float*)(wsb + ws.norm), out->sae_out, dY, (float*)(wsb + ws.loss_part), N, D,
                           grad_scale, ghost ? (float*)(gwb + gw.err) : (float*)nullptr, skip, gate, (ghost && tc) ? x : (const float*)nullptr,
                           split ? am(AM_DY) : (uint32_t*)nullptr);
        PV_LAUNCH_CHECK("dense_finish_kernel");
        sae_reduce_sum((const float*)(wsb + ws.loss_part), out->scalars, N, 1.0f / ((float)n_global * (float)sae_loss_width(d, st)), 1, -1,
                       stream, gate, 1u);
        if (ghost) {                                                  // the ghost loss and dHd, the part of d loss / d hidden_pre on the dead columns
            rc = ghost_residual(d, st, x, N, ghost, gw, out->scalars, 1.0f / ((float)n_global * (float)D), stream);
            if (rc) return rc;
        }
        hipLaunchKernelGGL(dense_loss_kernel, dim3(1), dim3(1), 0, stream, out->scalars, ghost ? 1 : 0, gate, 1u);
        // G4: gW_dec = f^T @ dY
        DenseGemm g4 = {};
        g4.A = f; g4.lda = F; g4.B = dY; g4.ldb = D; g4.M = F; g4.N = D; g4.K = N; g4.k_chunk = N;
        g4.out = st->gW_dec; g4.ldo = D; g4.gate = gate;
        if (split) { g4.a_max = am(AM_F); g4.b_max = am(AM_DY); }
        rc = launch_dense_gemm<true, true, DG_EPI_STORE>(g4, 1, stream);
        if (rc) return rc;
        if (nd > 0) {                                                 // gW_dec[dead] += exp(hidden_pre[:, dead])^T @ dG0
            rc = ghost_add_rows((const float*)(gwb + gw.dead_act), gw.n_pad, (const float*)(gwb + gw.dg0), gw.n_pad, N, st->gW_dec, ghost, gw, D, stream);
            if (rc) return rc;
        }
        // G3: dH = (dY @ W_dec^T + l1 / N) [f > 0], over f
        DenseGemm g3 = {};
        g3.A = dY; g3.lda = D; g3.B = st->W_dec; g3.ldb = D; g3.M = N; g3.N = F; g3.K = D; g3.k_chunk = D;
        g3.out = f; g3.ldo = F; g3.colpart = colpart; g3.add = l1_coefficient / (float)n_global; g3.gate = gate;
        if (split) { g3.a_max = am(AM_DY); g3.b_max = am(AM_WDEC); g3.amax_out = am(AM_DH); }
        g3.act = d.activation; g3.lp = d.lp_norm;
        if (lp_on) g3.lp_tok = (const float*)(wsb + ws.dense_lp_tok);
        if (nd > 0) { g3.dead_slot = ghost->dead_slot; g3.dead_act = (float*)(gwb + gw.dhd); g3.ldd = gw.n_pad; }      // + the ghost term
        rc = sae_plain_relu(d) ? launch_dense_gemm<false, false, DG_EPI_DH>(g3, 1, stream) : launch_dense_gemm<false, false, DG_EPI_DH_T>(g3, 1, stream);
        if (rc) return rc;
        rc = dense_colreduce(colpart, rblk, F, st->gb_enc, gate, stream);
        if (rc) return rc;
        // G5: gW_enc^T = dH^T @ sae_in
        DenseGemm g5 = {};
        g5.A = f; g5.lda = F; g5.B = sae_in; g5.ldb = D; g5.M = F; g5.N = D; g5.K = N; g5.k_chunk = N;
        g5.out = st->gW_enc; g5.ldo = D; g5.gate = gate;
        if (split) { g5.a_max = am(AM_DH); g5.b_max = am(AM_X); }
        rc = launch_dense_gemm<true, true, DG_EPI_STORE>(g5, 1, stream);
        if (rc) return rc;
    }
    return PV_OK;
}

// gb_dec = colsum(dY) - W_enc gb_enc (a transcoder: its two bias gradients, then gW_skip), from ws.dY and gb_enc of whichever form ran
int dense_bias_grads(const pv_sae_desc& d, const pv_sae_state* st, const float* x, int N, unsigned char* wsb, const SaeWs& ws, hipStream_t stream) {
    const float* dY = (const float*)(wsb + ws.dY);
    if (!sae_is_tc(st)) return sae_gbdec(d, st, dY, N, wsb, ws, stream, SAE_DY_TO_GB_DEC);
    const int rc = sae_gbdec(d, st, dY, N, wsb, ws, stream, SAE_DY_TO_GB_DEC_OUT);
    return rc ? rc : sae_tc_skip_backward(d, st, x, dY, N, stream);
}

// scalars[4] = l1_loss of the sparse form, scalars[5] = 0, scalars[0] = mse + l1 -- when the step ran sparse (*mode == 0)
__global__ __launch_bounds__(256) void relu_sparse_scalars_kernel(const float* __restrict__ l1part, int n, float scale,
                                                                  float* __restrict__ scalars, const uint32_t* __restrict__ mode) {
    __shared__ float red[4];
    if (*mode != 0u) return;
    float s = 0.f;
#pragma unroll 8
    for (int i = threadIdx.x; i < n; i += 256) s += l1part[i];        // (loads of 8 trips in flight, the sum in order)
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float l1 = ((red[0] + red[1]) + (red[2] + red[3])) * scale;
        scalars[4] = l1;
        scalars[5] = 0.f;
        scalars[0] = scalars[1] + l1;
    }
}
__global__ void set_u32_kernel(uint32_t* p, uint32_t v) { *p = v; }

// pv_sae_relu_step with the decoder renorm deferred (PV_SAE_RENORM_DECODER on a plan the sparse form covers): the sparse kernels use
// W_dec[j] * inv[j] on the fly; when the step turns out dense (*gate == 1) the five GEMMs read W_dec as it lies, so the rows are
// rewritten here -- the same products, stored -- and inv[j] = 1 tells pv_sae_apply that nothing is left to scale.  A wave per row.
__global__ __launch_bounds__(256) void relu_dense_renorm_kernel(float* __restrict__ W, float* __restrict__ inv, int rows, int d,
                                                                const uint32_t* __restrict__ gate) {
    if (*gate != 1u) return;
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= rows) return;
    const float s = inv[j];
    for (int c = 4 * lane; c < d; c += 256) {
        float4 w = *reinterpret_cast<const float4*>(W + (int64_t)j * d + c);
        w.x *= s; w.y *= s; w.z *= s; w.w *= s;
        *reinterpret_cast<float4*>(W + (int64_t)j * d + c) = w;
    }
    if (lane == 0) inv[j] = 1.0f;
}

// PV_SAE_SPARSE_GRADS on pv_sae_relu_step, behind a step that ran DENSE (gate == NULL: always; else *gate == 1): the gradient buffers
// are complete, so every feature is marked live for pv_sae_apply (offs[j] = j) and the per-feature terms of the clip norm, which the
// sparse backward leaves as a by-product, are taken from the rows here (rowsq[j] = |gW_dec[j]|^2 + |gW_enc^T[j]|^2 + gb_enc[j]^2).
__global__ __launch_bounds__(256) void relu_dense_live_kernel(const float* __restrict__ gW_dec, const float* __restrict__ gW_encT,
                                                              const float* __restrict__ gb_enc, uint32_t* __restrict__ offs,
                                                              float* __restrict__ rowsq, int rows, int d,
                                                              const uint32_t* __restrict__ gate) {
    if (gate && *gate != 1u) return;
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= rows) return;
    float sq = 0.f;
    for (int c = 4 * lane; c < d; c += 256) {
        const float4 a = *reinterpret_cast<const float4*>(gW_dec + (int64_t)j * d + c);
        const float4 b = *reinterpret_cast<const float4*>(gW_encT + (int64_t)j * d + c);
        sq += (a.x * a.x + a.y * a.y) + (a.z * a.z + a.w * a.w) + (b.x * b.x + b.y * b.y) + (b.z * b.z + b.w * b.w);
    }
    sq = wave_sum(sq);
    if (lane == 0) {
        const float gb = gb_enc[j];
        rowsq[j] = sq + gb * gb;
        offs[j] = (uint32_t)j;
        if (j == rows - 1) offs[rows] = (uint32_t)rows;
    }
}
}  // namespace
void sae_set_u32(uint32_t* p, uint32_t v, hipStream_t stream) { hipLaunchKernelGGL(set_u32_kernel, dim3(1), dim3(1), 0, stream, p, v); }

// One train step of the ReLU + L1 SAE on N tokens: forward + backward + statistics; gradients are WRITTEN into st->g*
// (complete buffers: pv_sae_grad_sqnorm and pv_sae_apply follow as usual).  scalars: 0 loss, 1 mse_loss, 2 l0, 4 l1_loss.
extern "C" int pv_sae_dense_step(pv_sae_plan* plan, pv_sae_state* st, const float* x, int32_t N, const float* batch_mean,
                                 int32_t n_global, int32_t flags, float l1_coefficient, const pv_sae_ghost* ghost, pv_sae_out* out,
                                 void* workspace, size_t workspace_bytes, void* stream_) {
    const int update_stats = (flags & PV_SAE_UPDATE_STATS) ? 1 : 0;
    int rc = dense_require(plan, st, x, N, n_global, update_stats, out, workspace, workspace_bytes);
    if (rc) return rc;
    const pv_sae_desc& d = plan->d;
    // ghost gradients (sae.py:151-179; train_sae.py:337-346): the caller lists the dead features (n_forward_passes_since_fired
    // > dead_feature_window BEFORE this step's statistics) and owns the extra workspace
    GhostWs gw = {};
    if (ghost) {
        PV_REQUIRE(n_global == N || (ghost->err_colmean && ghost->mse_global),
                   "ghost gradients with tokens sharded over ranks need pv_sae_ghost.err_colmean and mse_global (the global batch's)");
        rc = ghost_require(d, N, ghost, &gw);
        if (rc) return rc;
        // ghost gradients on a transcoder (round 6; transcoder.py:82-86): equal widths (the ghost residual is INPUT - sae_out), one process
        PV_REQUIRE(!sae_is_tc(st) || (st->tc.d_in_true <= 0 && st->tc.d_out_true <= 0 && n_global == N),
                   "transcoder + ghost gradients: d_out == d_in and the whole batch in one process");
    }
    const SaeWs ws = sae_carve(d);
    unsigned char* wsb = (unsigned char*)workspace;
    const float* skip = nullptr;
    rc = dense_prepare(plan, st, x, N, batch_mean, flags, false, wsb, ws, &skip, stream_);
    if (rc) return rc;
    rc = dense_step_body(plan, st, x, N, n_global, update_stats, l1_coefficient, ghost, gw, out, wsb, ws, skip, nullptr, (hipStream_t)stream_);
    return rc ? rc : dense_bias_grads(d, st, x, N, wsb, ws, (hipStream_t)stream_);
}

// The same step, sparse where the batch allows it ("ReLU is top-k with threshold 0 and a variable k", sae_enc_relu.hip: relu_select_kernel):
// ONE product over all features -- the fp16 filter with the threshold -B_n and the exact fp32 re-scoring of its survivors -- gives
// every token's positive activations as a list of at most sp->cap pairs; decode, CSR, the sparse backward and the bias gradients
// then run on the k-sparse kernels of sae.hip with k = cap (the L1 term: sum of the kept values; its gradient l1 / N on every kept
// pair).  A batch some token of which cannot be held (more positives than cap, a candidate slot overflow: the early, dense phase of
// training; the published x64 SAEs with L0 ~ 600-2000) raises the step's device-side mode word, the sparse kernels leave at once
// and the five dense GEMMs run instead -- decided on the GPU, no host round trip, same results either way (exact fp32 values on
// both paths).  sp == NULL or a plan the filter does not cover: the dense step.
extern "C" size_t pv_sae_relu_workspace_bytes(const pv_sae_plan* plan, int32_t n_tokens, int32_t cap) {
    if (!plan || n_tokens < 1 || cap < 4 || cap > PV_SAE_RELU_CAP_MAX || cap % 4) return 0;
    return relu_carve(plan->d, n_tokens, cap).total;
}

extern "C" size_t pv_debug_sae_relu_offset(const pv_sae_plan* plan, int32_t n_tokens, int32_t cap, const char* name) {
    if (!plan || !name || n_tokens < 1 || cap < 4 || cap > PV_SAE_RELU_CAP_MAX || cap % 4) return (size_t)-1;
    const ReluWs w = relu_carve(plan->d, n_tokens, cap);
    if (!strcmp(name, "mode")) return w.mode;
    if (!strcmp(name, "idx")) return w.idx;
    if (!strcmp(name, "val")) return w.val;
    if (!strcmp(name, "tok_cnt")) return w.tok_cnt;
    return (size_t)-1;
}

extern "C" int pv_sae_relu_step(pv_sae_plan* plan, pv_sae_state* st, const float* x, int32_t N, const float* batch_mean,
                                int32_t n_global, int32_t flags, float l1_coefficient, const pv_sae_relu_sparse* sp, pv_sae_out* out,
                                void* workspace, size_t workspace_bytes, void* stream_) {
    const int update_stats = (flags & PV_SAE_UPDATE_STATS) ? 1 : 0;
    int rc = dense_require(plan, st, x, N, n_global, update_stats, out, workspace, workspace_bytes);
    if (rc) return rc;
    const pv_sae_desc& d = plan->d;
    const SaeWs ws = sae_carve(d);
    unsigned char* wsb = (unsigned char*)workspace;
    hipStream_t stream = (hipStream_t)stream_;
    const bool tc = sae_is_tc(st);
    const bool sparse = sp && pv_sae_relu_sparse_ok(d) && sae_plain_relu(d) && st->W_enc16T && st->enc_colsq;      // (tanh-relu / lp_norm > 1: dense)
    // PV_SAE_SPARSE_GRADS (single-process training): a step that ran sparse leaves the rows of features no token kept unwritten, as
    // pv_sae_step does; a step that ran dense marks every feature live.  Either way pv_sae_grad_sqnorm_step / pv_sae_apply follow.
    const bool sparse_grads = (flags & PV_SAE_SPARSE_GRADS) != 0;
    // PV_SAE_RENORM_DECODER: deferred as in pv_sae_step where the sparse form applies (inverse norms now, the rows rewritten by
    // pv_sae_apply -- or here, in place, when the step turns out dense); otherwise W_dec is renormalised in place first
    const bool defer = sparse && (flags & PV_SAE_RENORM_DECODER) && st->dec_inv_norm;
    ReluWs rw = {};
    unsigned char* rwb = nullptr;
    if (sp) {
        PV_REQUIRE(sp->cap >= 4 && sp->cap <= PV_SAE_RELU_CAP_MAX && sp->cap % 4 == 0, "pv_sae_relu_sparse.cap: a multiple of 4 in [4, 256]");
        rw = relu_carve(d, N, sp->cap);
        PV_REQUIRE(sp->workspace && sp->workspace_bytes >= rw.total && ((uintptr_t)sp->workspace & 255) == 0,
                   "pv_sae_relu_sparse workspace too small / misaligned (pv_sae_relu_workspace_bytes)");
        rwb = (unsigned char*)sp->workspace;
    }
    const float* skip = nullptr;
    rc = dense_prepare(plan, st, x, N, batch_mean, defer ? (flags & ~PV_SAE_RENORM_DECODER) : flags, sparse, wsb, ws, &skip, stream_);
    if (rc) return rc;
    uint32_t* mode = sp ? (uint32_t*)(rwb + rw.mode) : nullptr;
    if (defer) {
        if (!(flags & PV_SAE_INV_NORM_VALID)) {
            rc = sae_dec_inv_norm(d, st, stream);
            if (rc) return rc;
        }
        plan->renorm_pending = true;
    }
    if (sparse) {
        const int cap = sp->cap;
        int32_t* idx = (int32_t*)(rwb + rw.idx);
        float* val = (float*)(rwb + rw.val);
        uint32_t* tok_cnt = (uint32_t*)(rwb + rw.tok_cnt);
        float* l1part = (float*)(rwb + rw.l1part);
        {
            ProfScope prof(PV_PROF_SAE_ENC, stream, 2.0 * N * (double)d.d_in * d.d_sae, ((double)N * d.d_in + (double)d.d_in * d.d_sae) * 2.0);
            rc = sae_encode_relu(d, st, N, cap, idx, val, tok_cnt, l1part, (uint32_t*)(rwb + rw.cand_cnt), rwb + rw.cand,
                                 (uint32_t*)(wsb + ws.cnt), (uint32_t*)(rwb + rw.wpos), mode, (const float*)out->scalars, wsb, ws, stream);
            if (rc) return rc;
        }
        rc = sae_sparse_tail(plan, st, x, N, n_global, cap, idx, val, out->sae_out, out->scalars, out->fire_count, update_stats,
                             sparse_grads, defer ? (const float*)st->dec_inv_norm : (const float*)nullptr, relu_tail(rwb, rw), wsb, ws,
                             tc ? (const float*)st->tc.target : x, tc ? (const float*)st->tc.b_dec_out : (const float*)st->b_dec, skip, tc,
                             l1_coefficient / (float)n_global, tok_cnt, mode, stream, /*bias_grads*/ false);
        if (rc) return rc;
        hipLaunchKernelGGL(relu_sparse_scalars_kernel, dim3(1), dim3(256), 0, stream, (const float*)l1part, N,
                           l1_coefficient / (float)n_global, out->scalars, (const uint32_t*)mode);
        PV_LAUNCH_CHECK("relu_sparse_scalars_kernel");
    } else if (mode) {
        sae_set_u32(mode, 1u, stream);
    }
    if (defer) {
        hipLaunchKernelGGL(relu_dense_renorm_kernel, dim3((d.d_sae + 3) / 4), dim3(256), 0, stream, st->W_dec, st->dec_inv_norm, d.d_sae,
                           d.d_in, (const uint32_t*)mode);
        PV_LAUNCH_CHECK("relu_dense_renorm_kernel");
    }
    rc = dense_step_body(plan, st, x, N, n_global, update_stats, l1_coefficient, nullptr, GhostWs{}, out, wsb, ws, skip, mode, stream);
    if (rc) return rc;
    rc = dense_bias_grads(d, st, x, N, wsb, ws, stream);      // once, behind both forms
    if (rc) return rc;
    if (sparse_grads) {
        uint32_t* offs = (uint32_t*)(wsb + ws.offs);
        hipLaunchKernelGGL(relu_dense_live_kernel, dim3((d.d_sae + 3) / 4), dim3(256), 0, stream, (const float*)st->gW_dec,
                           (const float*)st->gW_enc, (const float*)st->gb_enc, offs, (float*)(wsb + ws.rowsq), d.d_sae, d.d_in,
                           sparse ? (const uint32_t*)mode : (const uint32_t*)nullptr);
        PV_LAUNCH_CHECK("relu_dense_live_kernel");
        plan->live_offs = offs;
    }
    return PV_OK;
}
