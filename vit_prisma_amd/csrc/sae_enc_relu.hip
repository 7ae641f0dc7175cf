// ---------------------------------------------------------------------------------------------------
// ReLU encoder in sparse form (pv_sae_relu_step): f = relu(sae_in W_enc + b_enc) as per-token lists of its POSITIVE entries.
// "ReLU is top-k with threshold 0 and a variable k": the same fp16 filter GEMM runs with the per-token threshold -B_n (the
// error band of the fp16 product, see the file header: exact_j > 0  =>  a_j > -B_n), every survivor is re-scored EXACTLY in fp32
// against W_encT, and the ones whose exact value is positive are the token's activations -- values those of the exact fp32
// encoder.  A token's list holds at most `cap` pairs; a token with more positives than that, a candidate slot that overflowed or
// more than PV_SAE_CAND_CAP survivors raise the step's `mode` word: the step then runs on the dense GEMMs instead (sae_dense.hip, sae_gated.hip),
// so nothing is ever approximated.
// ---------------------------------------------------------------------------------------------------
// mode[0] = the step's mode word, mode[1] = dense steps in a row whose sparse attempt was skipped.  The attempt itself costs ~0.5 ms when
// it fails (one filter GEMM over all features): while the run is far from the sparse regime -- the previous step ran dense and kept more
// than twice the capacity per token on average (scalars[2] = its l0) -- the step goes dense at once (the filter GEMM and the selection
// leave on the raised word) and only every eighth such step probes.  Which form runs never changes a result.
// ("The file header" above is sae_enc.hip's: the derivation of B_n.  The filter GEMM is sae_enc_gemm.hip; the band, the candidate gather,
// the re-scoring and the ranking are the top-k form's own, sae_enc.hpp.)
#include "sae_enc.hpp"

namespace {

__global__ __launch_bounds__(256) void relu_thr_kernel(const float* __restrict__ xnorm, const float* __restrict__ wmax_sq, int d_in,
                                                       float* __restrict__ thr, int n_tok, uint32_t* __restrict__ mode,
                                                       const float* __restrict__ scalars, int cap) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n == 0) {
        const bool far = mode[0] == 1u && scalars && scalars[2] > 2.0f * (float)cap;
        const uint32_t streak = far ? mode[1] + 1u : 0u;
        mode[1] = streak;
        mode[0] = (far && (streak & 7u) != 0u) ? 1u : 0u;
    }
    if (n >= n_tok) return;
    const float B = enc_band(xnorm[n], *wmax_sq, d_in);
    thr[n] = (B == B) ? -B : -INFINITY;                        // (a NaN bound lets everything through: the slots overflow -> dense)
}

// One workgroup per token: candidates -> exact values -> the positive ones, ranked by (value desc, feature asc) -> idx / val /
// wpos [cap] (holes: val 0, wpos ~0), tok_cnt, the token's sum of activations (the L1 term).
// GATED (pv_sae_gated_step_sparse): b_enc = b_gate, the list = the features whose GATE is open (gate_pre = sae_in W_enc + b_gate > 0,
// sae.py:703-706), ranked by gate_pre.  A pair carries two values: val_out = feature_acts = relu(p e^r_mag + b_mag) (0 where the
// magnitude path is shut: such a pair still carries the gate path's gradient), valg_out = relu(gate_pre).  l0part = the token's count of
// feature_acts > 0.
template <int V4, bool GATED = false>
__global__ __launch_bounds__(256) void relu_select_kernel(
    const float* __restrict__ sae_in, const float* __restrict__ W_encT, const float* __restrict__ b_enc,
    const uint32_t* __restrict__ tile_cnt, const int2* __restrict__ cand, const float* __restrict__ thr, int32_t* __restrict__ idx_out,
    float* __restrict__ val_out, uint32_t* __restrict__ tok_cnt, float* __restrict__ l1part, uint32_t* __restrict__ feat_cnt,
    uint32_t* __restrict__ wpos, uint32_t* __restrict__ mode, int d, int cap, int ntn, int slots,
    const float* __restrict__ r_mag = nullptr, const float* __restrict__ b_mag = nullptr, float* __restrict__ l0part = nullptr,
    float* __restrict__ valg_out = nullptr) {
    __shared__ int32_t cidx[PV_SAE_CAND_CAP];
    __shared__ float rval[PV_SAE_CAND_CAP];
    __shared__ float rmag[GATED ? PV_SAE_CAND_CAP : 1];
    __shared__ uint32_t sh_l0;
    __shared__ uint32_t tcnt[256];
    __shared__ float sval[256];                              // the kept values in rank order (cap <= 256)
    __shared__ float red[4];
    __shared__ uint32_t sh_bad, sh_m;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row = blockIdx.x;
    // another token has already sent the step to the dense GEMMs: nothing this workgroup computes would be used (the mode word only
    // ever goes 0 -> 1 within a step; a stale 0 costs time, never correctness)
    if (tid == 0) { sh_bad = __hip_atomic_load(mode, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u ? 1u : 0u; sh_m = 0u; }
    __syncthreads();                                           // (ONE read of the word per workgroup: every thread sees the same answer)
    const bool already_dense = sh_bad != 0u;
    const EncSpan span = enc_cand_span(tile_cnt, row, ntn, tcnt, &sh_bad, already_dense, (uint32_t)PV_SAE_CAND_CAP);
    const uint32_t myc = span.myc, off = span.off, n = span.n;
    bool bad = span.bad;
    if (!bad && tid < ntn && myc > 0u) {
        // candidates whose filter value lies above +B_n are positive for certain (exact >= a - B_n > 0): more of those than the list
        // can hold settles the matter before a single row of W_enc is gathered (the published L0 of 600 - 2000 ends here)
        const int2* src = cand + (row * ntn + tid) * slots;
        const float Bn = -thr[row];
        uint32_t sure = 0;
        for (uint32_t e = 0; e < myc; ++e) {
            const int2 c = src[e];
            cidx[off + e] = c.x;
            sure += __int_as_float(c.y) > Bn ? 1u : 0u;
        }
        if (sure) atomicAdd(&sh_m, sure);
    }
    __syncthreads();
    if (!bad && sh_m > (uint32_t)cap) bad = true;
    __syncthreads();
    if (tid == 0) sh_m = 0u;
    const uint32_t nr = bad ? 0u : n;
    // exact fp32 re-scoring of every candidate
    enc_rescore<V4>(W_encT, sae_in + row * d, d, cidx, nr, wave, lane, [&](uint32_t c, int jv, float av) {
        rval[c] = av + b_enc[jv];
        if constexpr (GATED) rmag[c] = fmaxf(av * expf(r_mag[jv]) + b_mag[jv], 0.f);      // (as DG_EPI_GENC writes it)
    });
    __syncthreads();
    // how many are positive (NaN counts as not positive, like torch's relu keeps NaN -- a NaN pre-activation poisons the dense path
    // the same way: such a token is sent there)
    uint32_t mine = 0;
    bool nan_seen = false;
    for (uint32_t c = tid; c < nr; c += 256) {
        const float v = rval[c];
        mine += v > 0.f ? 1u : 0u;
        nan_seen = nan_seen || (v != v);
    }
    if (mine) atomicAdd(&sh_m, mine);
    if (nan_seen) sh_bad = 1u;
    __syncthreads();
    const uint32_t m = sh_m;
    bad = bad || sh_bad != 0u || m > (uint32_t)cap;
    auto holes_from = [&](int first) {                         // list positions first.. of the row: holes
        for (int s = first + tid; s < cap; s += 256) {
            idx_out[row * cap + s] = 0;
            val_out[row * cap + s] = 0.f;
            wpos[row * cap + s] = 0xffffffffu;
            if constexpr (GATED) valg_out[row * cap + s] = 0.f;
        }
    };
    if (bad) {                                                 // (uniform) this token cannot be held: the whole step goes dense
        if (tid == 0) {
            // (a workgroup that FOUND the word raised leaves it alone: at the published L0 every one of the 4096 does, and their
            // atomics on the one word were 40 of the 62 us this kernel took to do nothing)
            if (!already_dense) atomicOr(mode, 1u);
            tok_cnt[row] = 0u; l1part[row] = 0.f;
            if constexpr (GATED) l0part[row] = 0.f;
        }
        holes_from(0);
        return;
    }
    sval[tid] = 0.f;
    if (tid == 0) sh_l0 = 0u;
    __syncthreads();
    uint32_t myl0 = 0;
    for (uint32_t c = tid; c < nr; c += 256) {
        const float vc = rval[c];
        if (!(vc > 0.f)) continue;
        const int32_t ic = cidx[c];
        const uint32_t rank = enc_rank(rval, cidx, nr, vc, ic);
        const uint32_t wp = atomicAdd(&feat_cnt[ic], 1u);
        idx_out[row * cap + rank] = ic;
        wpos[row * cap + rank] = wp;
        if constexpr (GATED) {
            const float f = rmag[c];
            val_out[row * cap + rank] = f;
            valg_out[row * cap + rank] = vc;
            myl0 += f > 0.f ? 1u : 0u;
        } else {
            val_out[row * cap + rank] = vc;
        }
        sval[rank] = vc;
    }
    holes_from((int)m);                                        // the rest of the row
    if (GATED && myl0) atomicAdd(&sh_l0, myl0);
    __syncthreads();
    // the token's L1 term, summed in rank order (the candidates arrive in whatever order the filter's LDS atomics drew)
    const float lsum = wave_sum(sval[tid]);
    if (lane == 0) red[wave] = lsum;
    __syncthreads();
    if (tid == 0) {
        tok_cnt[row] = m;
        l1part[row] = (red[0] + red[1]) + (red[2] + red[3]);
        if constexpr (GATED) l0part[row] = (float)sh_l0;
    }
}
}  // namespace

int relu_select_occupancy(int* n) {
    PV_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(n, reinterpret_cast<const void*>(&relu_select_kernel<3, false>), 256, 0));
    return PV_OK;
}

int sae_encode_relu(const pv_sae_desc& d, const pv_sae_state* st, int N, int cap, int32_t* idx, float* val, uint32_t* tok_cnt,
                    float* l1part, uint32_t* cand_cnt, void* cand, uint32_t* feat_cnt, uint32_t* wpos, uint32_t* mode,
                    const float* prev_scalars, unsigned char* wsb, const SaeWs& ws, hipStream_t stream, float* l0part, float* valg) {
    // l0part != NULL: the gated form (see relu_select_kernel) -- the bias is b_gate, val = feature_acts, valg = relu(gate_pre)
    const bool gated = l0part != nullptr;
    const float* bias = gated ? (const float*)st->gt.b_gate : (const float*)st->b_enc;
    PV_REQUIRE(st->W_encT && st->W_enc16T && st->enc_colsq, "encoder shadows (W_encT, W_enc16T, enc_colsq) are required");
    PV_REQUIRE(cap >= 4 && cap <= PV_SAE_RELU_CAP_MAX && cap % 4 == 0, "cap");
    float* wmax = (float*)(wsb + ws.wmax);
    uint32_t* fb_count = (uint32_t*)(wsb + ws.fb_count);
    if (const int rc = launch_enc_wmax(st->enc_colsq, d.d_sae, wmax, fb_count, feat_cnt, stream)) return rc;
    hipLaunchKernelGGL(relu_thr_kernel, dim3((N + 255) / 256), dim3(256), 0, stream, (const float*)(wsb + ws.xnorm), (const float*)wmax,
                       d.d_in, (float*)(wsb + ws.thr), N, mode, prev_scalars, cap);
    PV_LAUNCH_CHECK("relu_thr_kernel");
    EncParams p = {};
    p.A = wsb + ws.x16; p.M = N; p.K = d.d_in; p.lda = d.d_in;
    p.B = st->W_enc16T; p.N = d.d_sae; p.ldb_bytes = (uint32_t)d.d_in * 2u; p.b_span = (uint32_t)d.d_sae * p.ldb_bytes;
    p.bias = bias; p.bias_stride = 1; p.out = nullptr; p.thr = (const float*)(wsb + ws.thr);
    p.cnt = cand_cnt; p.cand = (int2*)cand; p.slots = PV_SAE_RELU_SLOTS; p.mode = mode;
    int rc = launch_enc_gemm(1, p, stream);
    if (rc) return rc;
    const int ntn = d.d_sae / 256;
    auto select = [&](auto kernel) {                           // (not gated: the kernel's four gated pointers are null, as its defaults are)
        hipLaunchKernelGGL(kernel, dim3(N), dim3(256), 0, stream, (const float*)(wsb + ws.sae_in), (const float*)st->W_encT, bias,
                           (const uint32_t*)cand_cnt, (const int2*)cand, (const float*)(wsb + ws.thr), idx, val, tok_cnt, l1part, feat_cnt,
                           wpos, mode, d.d_in, cap, ntn, PV_SAE_RELU_SLOTS, gated ? (const float*)st->gt.r_mag : (const float*)nullptr,
                           gated ? (const float*)st->gt.b_mag : (const float*)nullptr, l0part, gated ? valg : (float*)nullptr);
    };
#define CALL(D)                                          \
    if (gated) select(relu_select_kernel<D, true>);      \
    else select(relu_select_kernel<D, false>)
    V4_DISPATCH(d.d_in, CALL);
#undef CALL
    PV_LAUNCH_CHECK("relu_select_kernel");
    return PV_OK;
}
