// The fp32 / split-fp16 GEMM of the dense SAE steps (sae_dense_gemm.hip): what a launch is told (DenseGemm), the operand maxima of the
// split-fp16 form, and the reduction of the epilogues' column partials.  Callers: sae_dense.hip, sae_ghost.hip, sae_gated.hip.
#pragma once
#include "sae.hpp"

constexpr int DG_KSLAB = 32;                  // floats of K per stage

enum { DG_EPI_STORE = 0, DG_EPI_ENC = 1, DG_EPI_DH = 2, DG_EPI_MUL = 3, DG_EPI_GENC = 4, DG_EPI_EXPB = 5,      // EXPB: out = exp(acc + bias)
       DG_EPI_ENC_T = 6, DG_EPI_DH_T = 7 };   // ENC / DH with the tail of SURVEY.md 8(f) row 3 compiled in: tanh-relu, lp_norm > 1 (DenseGemm.act / lp)

struct DenseGemm {
    const float* A; int64_t lda;              // A_KM ? [K][lda] (M contiguous) : [M][lda] (K contiguous)
    const float* B; int64_t ldb;              // B_KN ? [K][ldb] (N contiguous) : [N][ldb] (K contiguous)
    int M, N, K;
    int k_chunk;                              // K range of one blockIdx.y (multiple of 32; K when not split)
    int group;                                // set by the launcher: row tiles per group of the tile order (see the kernel), 0 = N fastest
    float* out; int64_t ldo;                  // STORE: out + blockIdx.y * out_zstride
    int64_t out_zstride;
    const float* bias;                        // ENC: b_enc [N]
    float* colpart;                           // ENC / DH: [ceil(M / 64)][N] column partials of the wave's 64-row block
    float* rowpart;                           // ENC: [ceil(M / 64)][ceil(N / 64)] sums of f over the wave's 64 x 64 block
    float add;                                // DH: l1_coefficient / N_global
    // ghost gradients (sae.py:151-179): the dead features' columns, compacted
    const int32_t* dead_slot;                 // ENC / DH: [N] column -> compact slot of a dead feature, -1 otherwise; or NULL
    float* dead_act; int64_t ldd;             // ENC: exp(hidden_pre) of the dead columns -> dead_act[row][slot];  DH: the ghost term of
                                              //      d loss / d hidden_pre, added to dH there
    const float* mul;                         // MUL: out = acc * mul (same shape and leading dimension as out)
    // gated SAE (sae.py:699-716): GENC takes acc = sae_in @ W_enc and writes feature_acts = [acc + bias > 0] relu(acc e^cscale + bias2)
    // to out, relu(acc + bias) to out2 (same leading dimension); colpart = firing counts, colpart2 / rowpart = sums of out2.
    // DH with colpart2: additionally the column sums of dH * (the stored activation) (the gradient of r_mag)
    const float* bias2;
    const float* cscale;
    float* out2;
    float* colpart2;
    // pv_sae_relu_step: the step's mode word (device).  Non-NULL: the kernel runs only when *gate == 1 (the sparse attempt could not
    // hold the batch); NULL: always.
    const uint32_t* gate;
    // split-fp16 form (SPLIT kernels, round 6): DG_AMAX_SLOTS words each -- the bit patterns of partial maxima of |A| and |B| (any entry
    // may be 0); the largest gives the operand's power-of-two scale.  amax_out (ENC / GENC / DH epilogues, or NULL): the same for the
    // tensor this launch writes to `out` (atomicMax on bit patterns of non-negative floats: order-independent, so run-to-run identical)
    const uint32_t* a_max;
    const uint32_t* b_max;
    uint32_t* amax_out;
    // round 6: the tail of SURVEY.md 8(f) row 3 on the ENC / DH epilogues
    int act;                                  // PV_SAE_ACT_TANH_RELU: f = tanh(relu(.)) (sae.py:823-830); DH: x (1 - f^2)
    float lp;                                 // p of the sparsity term ||f_n||_p (sae.py:617); 0 / 1: the 1-norm
    float* lp_part;                           // ENC, lp > 1: [M][ceil(N / 64)] sums of f^p over the row's 64 columns of a wave
    const float* lp_tok;                      // DH, lp > 1: [M] l1 / N_global * ||f_n||_p^(1 - p), the per-token factor of d ||f_n||_p / d f
};

// the split-fp16 form when the launch carries both operand maxima (and dense_fp32 is off), else the exact fp32 one; the ten forms in use
template <bool A_KM, bool B_KN, int EPI>
int launch_dense_gemm(const DenseGemm& p, int splits, hipStream_t stream);

// ---- operand maxima of the split-fp16 form: DG_AMAX_SLOTS partial maxima per tensor, tensor t at SaeWs.dense_amax + t * DG_AMAX_SLOTS words
constexpr int DG_AMAX_SLOTS = 256;
enum { DG_AM_X = 0, DG_AM_WENC = 1, DG_AM_WDEC = 3 };      // the three operands that exist before a step's first GEMM; the rest are the step's own
struct DenseAmax { uint32_t* base; uint32_t* operator()(int t) const { return base + t * DG_AMAX_SLOTS; } };      // am(t): tensor t's slots
// do a step's GEMMs run in the split-fp16 form?  (16-byte rows of every operand; the tuning key dense_fp32 forces the exact form)
static inline bool dense_split_ok(const pv_sae_desc& d, int N) {
    return !g_pv_tuning.dense_fp32 && (d.d_in % 4) == 0 && (d.d_sae % 4) == 0 && (N % 4) == 0;
}
// the head of a split-fp16 step: every slot array zeroed, then the maxima of sae_in, W_enc^T and W_dec in one launch
int dense_absmax3(const pv_sae_desc& d, const pv_sae_state* st, const float* sae_in, int N, uint32_t* amax, const uint32_t* gate, hipStream_t stream);

// column partials [nblk][d] of an ENC / GENC / DH epilogue -> out[j], in block order; the first form also keeps the firing statistics
// (train_sae.py:356-361) and leaves the sum of each 256 columns in blk_tot (l0)
int dense_colreduce(const float* part, int nblk, int d, float* out, float* act_freq, float* n_since_fired, int update_stats, float* blk_tot,
                    const uint32_t* gate, hipStream_t stream);
int dense_colreduce(const float* part, int nblk, int d, float* out, const uint32_t* gate, hipStream_t stream);
