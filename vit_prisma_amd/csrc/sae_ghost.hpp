// Ghost gradients (SparseAutoencoder._compute_ghost_residual_loss, sae.py:151-179), sae_ghost.hip: what the dense ReLU + L1 step
// (sae_dense.hip) and the pass behind a top-k step (pv_sae_topk_ghost) share.
#pragma once
#include "sae_dense_gemm.hpp"

struct GhostWs {                              // offsets into pv_sae_ghost.workspace; n_pad: n_dead rounded up to a multiple of 8
    size_t total, dead_act, dhd, wdd, g0, dg0, err, tmpw, colmean, part, colpart, vec_a, vec_b, colpart_p;
    int n_pad;
};
// the checks of pv_sae_ghost that do not depend on the step, and the carve
int ghost_require(const pv_sae_desc& d, int N, const pv_sae_ghost* ghost, GhostWs* gw);
// From exp(hidden_pre[:, dead]) (gw.dead_act [N][n_pad]) and err = sae_out - x (gw.err): G0 = act @ W_dec[dead], the ghost loss (scalars[5];
// rescaled by the mse in scalars[1], a transcoder's by scalars[7], taken here on x = its input), d loss / d G0 per token (gw.dg0) and what
// reaches hidden_pre of the dead features, dHd = (dG0 @ W_dec[dead]^T) * act (gw.dhd).  inv_cnt = 1 / (N_global d_in).
int ghost_residual(const pv_sae_desc& d, const pv_sae_state* st, const float* x, int N, const pv_sae_ghost* ghost, const GhostWs& gw,
                   float* scalars, float inv_cnt, hipStream_t stream);
// dst[dead_idx[s]] += (A^T @ B)[s] for s < n_dead: A [K][lda] with M = n_pad columns, B [K][d_in]; the product goes through gw.tmpw
int ghost_add_rows(const float* A, int64_t lda, const float* B, int M, int K, float* dst, const pv_sae_ghost* ghost, const GhostWs& gw, int d_in,
                   hipStream_t stream);
