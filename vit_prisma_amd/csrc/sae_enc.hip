// SAE encoder + TopK without materialising hidden_pre (gfx950).
//
// Reference semantics: hidden_pre = sae_in @ W_enc + b_enc (sae/sae.py:567-574), TopK keeps the k largest per token
// (sae/sae.py:795-810).  Only k = 32 of the d_sae = 24 576 pre-activations of a token survive, so the [N, d_sae] fp32
// matrix (403 MB at N = 4096) is never written.  Instead:
//
//   pass 0   filter GEMM on every 16th feature (fp16 MFMA, 1/16 of the work) -> sample [N, d_sae/16]
//   thr      per token: s_q = q-th largest sampled value (q = 12 for k = 32).  Any q values bound the k-th largest of
//            the full row from below unless q of the true top-k happen to sit in the sample (2e-7 per token), so
//            T_n = s_q - 2 B_n is a threshold that ~16 q = 190 of the 24 576 values pass
//   filter   the full encoder product on v_mfma_f32_32x32x16_f16 (operands rounded to fp16: a_j = approx hidden_pre,
//            |a_j - exact| <= B_n, see below); the epilogue keeps no tile -- it appends (j, a_j) for a_j >= T_n to the
//            token's candidate list (one atomic per hit, ~0.8 % of the elements)
//   select   per token: t = k-th largest a; if t >= s_q every feature with a_j >= t - 2 B_n is in the list, and that set
//            contains the exact top-k.  Those (~k + 7) candidates are re-scored EXACTLY in fp32 against a transposed
//            fp32 copy of W_enc (coalesced 3 KB rows) and ranked by (value desc, index asc): index sets and values are
//            those of the exact-fp32 path
//   fallback tokens the filter cannot decide (t < s_q, list overflow = massive ties, > 192 candidates in the band,
//            fp16 overflow) are recomputed exactly (fp32 row into the hidden scratch + the streaming / radix top-k of
//            sae.hip).  Expected: none on ordinary data; everything on adversarial data; never a wrong answer.
//
// Error bound of the filter (x = sae_in row, w = W_enc column, K = d_in; fp16 has an 11-bit significand, u = 2^-11):
//   |x.w - fl16(x).fl16(w)| <= (2u + u^2) sum|x_i w_i| + 2^-25 (sum|x_i| + sum|w_i|)      (operand rounding, subnormals)
//   fp32 accumulation of exact products on the matrix core, and the fp32 re-scoring it is compared with:
//                           <= 4 K 2^-24 sum|x_i w_i| + K 2^-24 sum|x_i w_i|
//   => B_n = ||x_n||_2 (C1 Wmax + C2) + C2 Wmax,  C1 = max(1.25e-3, 2^-10 (1 + 2^-12) + 5 K 2^-24) (enc_c1(K): 1.25e-3 up to K = 916,
//      1.36e-3 at K = 1280),
//      C2 = 2^-25 sqrt(K),  Wmax = max_j ||W_enc[:, j]||_2 (maintained by the Adam kernel as enc_colsq).
//   The two compared values are each acc + b_enc[j] rounded once to fp32: 2 x 2^-24 |a_j|, covered by a rounding term 4.8e-7 |v| on top of
//   B_n, v being the size of the sums compared.  sae_thr_kernel knows s_q (the q-th largest SAMPLED value) and leaves 2 B_n(|s_q|) in band[];
//   sae_select_kernel compares around t, the k-th largest filter value, and adds 9.6e-7 (|t| - |s_q|) where that is positive.  (Until the
//   planted suite, tests/_sae_encoder_cases.py ``bias_dominated``, the band around t carried the term at |s_q| only: nine features with
//   b_enc = 2^20 off the sample, sampled values near 1 -- the exact largest came back one fp32 step of 2^20 below t in the filter,
//   300 bands away, was never re-scored, and the row returned a wrong index set with no fallback.)  The threshold needs no such change:
//   v - 2 c |v| increases with v, so t >= s_q gives t - 2 B_n(|t|) >= s_q - 2 B_n(|s_q|) = T_n and the band below t is in the list.
//   The same suite holds the band to its factor: rows whose loser beats the winner by 1.05 B_n in the filter (operand rounding on disjoint
//   halves of x reaches 1.1 B_n at most) lose a winner under a band of B_n or a C1 below 2^-10, at d_in 64 and at 1032 where enc_c1
//   leaves its floor.  The ReLU threshold -B_n needs no rounding term: fl32 is monotone, so exact_j > 0 implies a_j >= fl32(-B_n).
// Rows with |x| beyond the fp16 range get B = inf (-> fallback); a weight beyond it makes its column norm inf (-> every
// row falls back): slow, never wrong.
//
// This file: the top-k form (thr, select, fallback).  The filter GEMM is sae_enc_gemm.hip, the sparse ReLU / gated form sae_enc_relu.hip;
// what the two forms share (the band, the candidate gather, the re-scoring, the ranking) is sae_enc.hpp.
#include "sae_enc.hpp"

namespace {

// ---------------------------------------------------------------------------------------------------
// thr: q-th largest of a token's sampled values, band and threshold.  One wave per token.
// ---------------------------------------------------------------------------------------------------
template <int VPL>                                            // sampled values per lane: ns <= 64 VPL
__global__ __launch_bounds__(256) void sae_thr_kernel(const float* __restrict__ sample, int ns, const float* __restrict__ xnorm,
                                                      const float* __restrict__ wmax_sq, int qsel, int d_in, float* __restrict__ thr,
                                                      float* __restrict__ sq_out, float* __restrict__ band, int n_tok,
                                                      int nb_thr, const float* __restrict__ cs_partial, float* __restrict__ cs_out,
                                                      int cs_nblk, float cs_scale) {
    // workgroups beyond nb_thr (the fused pre-pass, SaePre): the batch mean's second stage -- 16 columns each
    if ((int)blockIdx.x >= nb_thr) {
        colsum_final_body_256(blockIdx.x - nb_thr, cs_partial, cs_out, cs_nblk, d_in, cs_scale);
        return;
    }
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= n_tok) return;
    const float* s = sample + (int64_t)n * ns;
    float v[VPL];
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int c = lane + 64 * i;
        v[i] = c < ns ? s[c] : -INFINITY;
        v[i] = (v[i] == v[i]) ? v[i] : -INFINITY;             // NaN never bounds anything
    }
    // The q-th largest of a SUBSET of the row's values bounds the k-th largest of the row from below like the q-th largest of the whole
    // sample does (file header), only a hair lower where the subset misses one of the sample's top q.  The subset: every lane's three
    // largest (192 values; a lane holds four of the sample's top 12 about once in 10^4 tokens) -- kept sorted in three registers while
    // the lane's values stream by, so that a selection round is a wave maximum and a pop instead of a pass over all VPL registers
    // (the exact form took 12 rounds x (VPL maxima + VPL compare-and-clear): 20 us of the step; this one 9).  Multiplicity counts.
    float t0 = -INFINITY, t1 = -INFINITY, t2 = -INFINITY;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const float x = v[i];
        const float a = fmaxf(t0, x), b = fminf(t0, x);        // (t0, t1, t2, x) -> the three largest, in order
        const float c = fmaxf(t1, b), e = fminf(t1, b);
        t0 = a; t1 = c; t2 = fmaxf(t2, e);
    }
    float m = -INFINITY;
    for (int rnd = 0; rnd < qsel; ++rnd) {
        m = wave_max(t0);
        const unsigned long long owners = __ballot(t0 == m);
        const int owner = __ffsll((long long)owners) - 1;
        if (lane == owner) { t0 = t1; t1 = t2; t2 = -INFINITY; }      // remove ONE instance
    }
    if (lane == 0) {
        const float B = enc_band(xnorm[n], *wmax_sq, d_in) + 4.8e-7f * fabsf(m);
        sq_out[n] = m;
        band[n] = 2.0f * B;
        thr[n] = m - 2.0f * B;
    }
}

// the weight bound where no prep launch carries it (sae_prep_roles_kernel, sae.hip, runs the same body as its workgroup 0)
__global__ __launch_bounds__(256) void sae_wmax_kernel(const float* __restrict__ colsq, int d_sae, float* __restrict__ out,
                                                       uint32_t* __restrict__ fb_count, uint32_t* __restrict__ feat_cnt) {
    enc_wmax_body(colsq, d_sae, out, fb_count, feat_cnt);
}

// ---------------------------------------------------------------------------------------------------
// select: candidates -> exact top-k.  One workgroup per token.
// ---------------------------------------------------------------------------------------------------
#ifndef PV_SEL_WAVES
#define PV_SEL_WAVES 8        // waves per SIMD the select kernel is compiled for (see the kernel)
#endif
// The k-th largest (with multiplicity) of nc <= 64 KPL ordered keys in LDS, by ONE wave: KPL keys per lane in registers, a radix select
// from the highest bit in which the keys differ -- a ballot + popcount per key and bit -- that stops as soon as the survivors are exactly
// the ones still wanted (~10 bits on ordinary data).  Every lane returns the key.
template <int KPL>
__device__ __forceinline__ uint32_t sel_radix_kth(const uint32_t* ckey, uint32_t nc, uint32_t k, int lane) {
    uint32_t key[KPL];
    uint32_t alive = 0u;
#pragma unroll
    for (int i = 0; i < KPL; ++i) {
        const uint32_t c = (uint32_t)lane + 64u * i;
        key[i] = c < nc ? ckey[c] : 0u;
        alive |= c < nc ? (1u << i) : 0u;
    }
    auto alive_minmax = [&](uint32_t& mn, uint32_t& mx) {
        mn = 0xffffffffu; mx = 0u;
#pragma unroll
        for (int i = 0; i < KPL; ++i)
            if (alive & (1u << i)) { mn = min(mn, key[i]); mx = max(mx, key[i]); }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mn = min(mn, (uint32_t)__shfl_xor((int)mn, o, 64));
            mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, 64));
        }
    };
    uint32_t kmin, kmax;
    alive_minmax(kmin, kmax);
    uint32_t krem = k, n_alive = nc;
    if (kmin != kmax) {
        for (int b = 31 - __clz((int)(kmin ^ kmax)); b >= 0; --b) {       // (everything below is wave-uniform)
            uint32_t cnt = 0;
#pragma unroll
            for (int i = 0; i < KPL; ++i)
                cnt += (uint32_t)__popcll(__ballot(((alive >> i) & 1u) != 0u && ((key[i] >> b) & 1u) != 0u));
            const bool take1 = cnt >= krem;                               // the k-th largest has this bit set
#pragma unroll
            for (int i = 0; i < KPL; ++i)
                if ((((key[i] >> b) & 1u) != 0u) != take1) alive &= ~(1u << i);
            if (take1) n_alive = cnt;
            else { krem -= cnt; n_alive -= cnt; }
            if (n_alive == krem || krem == 1u) break;
        }
        alive_minmax(kmin, kmax);
    }
    // survivors == wanted: the smallest of them; one wanted (or all survivors equal): the largest
    return n_alive == krem ? kmin : kmax;
}

// the same for any nc <= 1024 (PV_SAE_CAND_CAP): the keys stay in LDS, a 16-bit mask per lane says which of its (up to 16) keys are alive
__device__ __forceinline__ uint32_t sel_radix_kth_lds(const uint32_t* ckey, uint32_t nc, uint32_t k, int lane) {
    const int nk = (int)((nc + 63u) >> 6);                     // keys per lane (wave-uniform)
    uint32_t alive = 0u;
    for (int i = 0; i < nk; ++i) alive |= ((uint32_t)lane + 64u * i) < nc ? (1u << i) : 0u;
    auto alive_minmax = [&](uint32_t& mn, uint32_t& mx) {
        mn = 0xffffffffu; mx = 0u;
        for (int i = 0; i < nk; ++i)
            if (alive & (1u << i)) { const uint32_t key = ckey[lane + 64 * i]; mn = min(mn, key); mx = max(mx, key); }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mn = min(mn, (uint32_t)__shfl_xor((int)mn, o, 64));
            mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, 64));
        }
    };
    uint32_t kmin, kmax;
    alive_minmax(kmin, kmax);
    uint32_t krem = k, n_alive = nc;
    if (kmin != kmax) {
        for (int b = 31 - __clz((int)(kmin ^ kmax)); b >= 0; --b) {       // (everything below is wave-uniform)
            uint32_t cnt = 0, ones = 0u;
            for (int i = 0; i < nk; ++i) {
                const bool one = ((alive >> i) & 1u) != 0u && ((ckey[lane + 64 * i] >> b) & 1u) != 0u;
                cnt += (uint32_t)__popcll(__ballot(one));
                ones |= one ? (1u << i) : 0u;
            }
            const bool take1 = cnt >= krem;                               // the k-th largest has this bit set
            alive = take1 ? ones : (alive & ~ones);
            if (take1) n_alive = cnt;
            else { krem -= cnt; n_alive -= cnt; }
            if (n_alive == krem || krem == 1u) break;
        }
        alive_minmax(kmin, kmax);
    }
    return n_alive == krem ? kmin : kmax;
}

#ifdef PV_SEL_TRACE       // (debug build, tools/build_variant.sh: per-workgroup time stamps of the select kernel into the hidden scratch -- 100 MHz wall clock)
#define SEL_STAMP(slot)                                                                                                   \
    do {                                                                                                                  \
        if (hidden && threadIdx.x == 0) {                                                                                 \
            uint64_t* tr = reinterpret_cast<uint64_t*>(hidden);                                                           \
            tr[(int64_t)blockIdx.x * 4 + (slot)] = wall_clock64();                                                        \
            if ((slot) == 0) tr[(int64_t)blockIdx.x * 4 + 3] = ((uint64_t)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32) | \
                                                              (uint64_t)__builtin_amdgcn_s_getreg((31 << 11) | 4);        \
        }                                                                                                                 \
    } while (0)
#else
#define SEL_STAMP(slot) do { } while (0)
#endif
// INLINE_FB (the folded training step): a token the filter cannot decide is recomputed exactly by ITS OWN workgroup, right here -- the
// row of exact pre-activations in sae_fb_hidden_kernel's arithmetic (a wave per feature, the same fma chain, wave_sum), then
// sae_topk_row_lds on the LDS of the candidate pass -- instead of being listed for the two fallback launches, which cost 9 us + two
// dispatch gaps per step when their list is empty, i.e. on every step of ordinary data.  A workgroup that takes the exact path runs
// ~0.3 ms (24 576 x 768 fp32 MACs on four waves); a batch in which EVERY token does (adversarial data) takes about as long as the
// 32 x 24 workgroups of the listed form did.
template <int V4, bool INLINE_FB = false>
__global__ __launch_bounds__(256, PV_SEL_WAVES) void sae_select_kernel(
    const float* __restrict__ sae_in, const float* __restrict__ W_encT, const float* __restrict__ b_enc,
    const uint32_t* __restrict__ tile_cnt, const int2* __restrict__ cand, const float* __restrict__ sq,
    const float* __restrict__ band, int32_t* __restrict__ idx_out, float* __restrict__ val_out, int32_t* __restrict__ fb_list,
    uint32_t* __restrict__ fb_count, uint32_t* __restrict__ feat_cnt, uint32_t* __restrict__ wpos, int d, int k, int ntn, int slots,
    const float* __restrict__ xn = nullptr, const float* __restrict__ batch_mean = nullptr, float* __restrict__ norm_out = nullptr,
    int d_true = 0, float* __restrict__ hidden = nullptr) {
    __shared__ uint32_t ckey[PV_SAE_CAND_CAP];
    __shared__ int32_t cidx[PV_SAE_CAND_CAP];
    __shared__ int32_t ridx[PV_SAE_RESCORE_MAX];
    __shared__ float rval[PV_SAE_RESCORE_MAX];
    __shared__ uint32_t tcnt[256];
    __shared__ uint32_t sh_t, sh_nr, sh_bad;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row = blockIdx.x;
    SEL_STAMP(0);
    // (the fused pre-pass, SaePre) the loss normaliser ||x_n - mean_batch(x)||_2 that prep left out because the mean was not there yet:
    // sae_prep_kernel's loop in its order, on the wave that has nothing to do while the candidate lists are gathered.  The loads leave
    // here; they are used behind the candidate pass (the first barrier of the kernel would otherwise wait for this wave's HBM trip)
    float nx[4 * V4], nb[4 * V4];
    const bool norm_wave = xn != nullptr && wave == 3;
    if (norm_wave) {
        const float* xr = xn + row * d;
#pragma unroll
        for (int u = 0; u < 4 * V4; ++u) {
            const int i = lane + 64 * u;
            nx[u] = i < d_true ? xr[i] : 0.f;
            nb[u] = i < d_true ? batch_mean[i] : 0.f;
        }
    }
    // gather the token's candidates (enc_cand_span, sae_enc.hpp)
    if (tid == 0) { sh_t = 0u; sh_nr = 0u; sh_bad = 0u; }
    const EncSpan span = enc_cand_span(tile_cnt, row, ntn, tcnt, &sh_bad, false, ~0u);
    const uint32_t myc = span.myc, off = span.off, n = span.n;
    bool bad = span.bad || n > (uint32_t)PV_SAE_CAND_CAP || n < (uint32_t)k;
    if (!bad && tid < ntn && myc > 0u) {
        const int2* src = cand + (row * ntn + tid) * slots;
        // (the usual list is 1-4 entries: two independent 16-byte loads instead of a dependent chain)
        const int4 e01 = *reinterpret_cast<const int4*>(src), e23 = *reinterpret_cast<const int4*>(src + 2);
        const int2 first[4] = {{e01.x, e01.y}, {e01.z, e01.w}, {e23.x, e23.y}, {e23.z, e23.w}};
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if ((uint32_t)e < myc) {
                ckey[off + e] = pv_f2ord(__int_as_float(first[e].y));
                cidx[off + e] = first[e].x;
            }
        for (uint32_t e = 4; e < myc; ++e) {
            const int2 c = src[e];
            ckey[off + e] = pv_f2ord(__int_as_float(c.y));
            cidx[off + e] = c.x;
        }
    }
    const uint32_t nc = bad ? 0u : n;
    __syncthreads();
    // t = the k-th largest filter value (with multiplicity).  Round 3 ranked every candidate against every other out of LDS
    // (~190 x 190 compares per token: 75 of the kernel's 133 us, measured by running the pass twice); now ONE wave runs a radix
    // select over the ordered keys in registers -- four keys per lane, a ballot + popcount per key and bit, starting below the
    // keys' common prefix and stopping as soon as the survivors are exactly the ones still wanted (~10 bits on ordinary data) --
    // while the other waves wait at the barrier.  More than 256 candidates (heavy ties, small d_sae): the all-pairs ranking.
    if (!bad && wave == 0) {
        // (up to 256 candidates: four keys per lane in registers; more -- 1 % of the bench batch's tokens, which an all-pairs ranking
        // out of LDS kept in this kernel for 55 us while the others were done in 10, the kernel's tail -- the same select with the keys
        // re-read from LDS in every bit round: sixteen reads per lane and bit at the list's capacity)
        uint32_t kth;
        if (nc <= 256u) kth = sel_radix_kth<4>(ckey, nc, (uint32_t)k, lane);
        else kth = sel_radix_kth_lds(ckey, nc, (uint32_t)k, lane);
        if (lane == 0) sh_t = kth;
    }
    __syncthreads();
    const float t = pv_ord2f(sh_t);
    bad = bad || !(t >= sq[row]);                              // band below t not guaranteed to be in the list (or NaN)
    // the band's rounding term (file header) as sae_thr_kernel left it covers sums the size of s_q; the sums compared here are the size
    // of t, which is far larger where the row's large values come from b_enc and sit off the sample
    const float lo = t - (band[row] + 9.6e-7f * fmaxf(fabsf(t) - fabsf(sq[row]), 0.f));
    if (!bad) {
        for (uint32_t c = tid; c < nc; c += 256) {
            if (pv_ord2f(ckey[c]) >= lo) {
                const uint32_t pos = atomicAdd(&sh_nr, 1u);
                if (pos < (uint32_t)PV_SAE_RESCORE_MAX) ridx[pos] = cidx[c];
            }
        }
    }
    __syncthreads();
    const uint32_t nr = sh_nr;
    bad = bad || nr > (uint32_t)PV_SAE_RESCORE_MAX;
    SEL_STAMP(2);                                              // (candidate pass + threshold select done)
    if (norm_wave) {
        float cn = 0.f;
#pragma unroll
        for (int u = 0; u < 4 * V4; ++u) {                     // (terms beyond d_true are exact zeros: they do not move the sum)
            const float c = nx[u] - nb[u];
            cn += c * c;
        }
        cn = wave_sum(cn);
        if (lane == 0) norm_out[row] = sqrtf(cn);
    }
    if (bad) {                                                 // (uniform over the workgroup)
        if constexpr (!INLINE_FB) {
            if (tid == 0) fb_list[atomicAdd(fb_count, 1u)] = (int32_t)row;
            return;
        } else {
            if (tid == 0) atomicAdd(fb_count, 1u);             // (the count stays: NativeSAE.fallback_rows)
            const int d_sae = ntn * 256;
            float4 xq[V4];
#pragma unroll
            for (int i = 0; i < V4; ++i)
                xq[i] = 4 * lane + 256 * i < d ? *reinterpret_cast<const float4*>(sae_in + row * d + 4 * lane + 256 * i)
                                               : make_float4(0.f, 0.f, 0.f, 0.f);
            for (int j0 = wave * 4; j0 < d_sae; j0 += 16) {
                float acc[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float* w = W_encT + (int64_t)(j0 + u) * d;
                    float a = 0.f;
#pragma unroll
                    for (int i = 0; i < V4; ++i) {
                        if (4 * lane + 256 * i < d) {
                            const float4 wv = *reinterpret_cast<const float4*>(w + 4 * lane + 256 * i);
                            a = fmaf(xq[i].x, wv.x, a); a = fmaf(xq[i].y, wv.y, a); a = fmaf(xq[i].z, wv.z, a); a = fmaf(xq[i].w, wv.w, a);
                        }
                    }
                    acc[u] = a;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[u] = wave_sum(acc[u]);
                if (lane < 4) {
                    const float av = lane == 0 ? acc[0] : (lane == 1 ? acc[1] : (lane == 2 ? acc[2] : acc[3]));
                    hidden[row * d_sae + j0 + lane] = av + b_enc[j0 + lane];
                }
            }
            __threadfence_block();
            __syncthreads();                                   // the row is in memory for the whole workgroup
            sae_topk_row_lds(hidden, idx_out, val_out, d_sae, k, row, feat_cnt, wpos, tcnt, ckey, cidx);
            return;
        }
    }
    enc_rescore<V4>(W_encT, sae_in + row * d, d, ridx, nr, wave, lane, [&](uint32_t c, int jv, float av) { rval[c] = av + b_enc[jv]; });
    __syncthreads();
    for (uint32_t c = tid; c < nr; c += 256) {
        const float vc = rval[c];
        const int32_t ic = ridx[c];
        const uint32_t rank = enc_rank(rval, ridx, nr, vc, ic);
        if (rank < (uint32_t)k) {
            const float v = fmaxf(vc, 0.f);                    // postact_fn = ReLU (sae.py:806)
            idx_out[row * k + rank] = ic;
            val_out[row * k + rank] = v;
            // position of this pair in its feature's list (CSR of the backward), drawn while the result is written
            if (feat_cnt) wpos[row * k + rank] = v > 0.f ? atomicAdd(&feat_cnt[ic], 1u) : 0xffffffffu;
        }
    }
#ifdef PV_SEL_TRACE
    __syncthreads();
    SEL_STAMP(1);
#endif
}

// exact fp32 hidden_pre rows of the tokens the filter could not decide -> hidden scratch.  Reads W_enc as W_encT (the fp32
// master the Adam kernel keeps; the parameter's own layout may be stale): a wave per feature, the 3 KB row coalesced against
// the token's row in LDS.
__global__ __launch_bounds__(256) void sae_fb_hidden_kernel(const float* __restrict__ sae_in, const float* __restrict__ W_encT,
                                                            const float* __restrict__ b_enc, const int32_t* __restrict__ fb_list,
                                                            const uint32_t* __restrict__ fb_count, float* __restrict__ hidden,
                                                            int d, int d_sae) {
    __shared__ float xs[1280];
    const uint32_t nfb = *fb_count;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int jper = (d_sae + gridDim.y - 1) / gridDim.y;
    const int j_lo = blockIdx.y * jper, j_hi = min(d_sae, j_lo + jper);
    for (uint32_t s = blockIdx.x; s < nfb; s += gridDim.x) {
        const int64_t row = fb_list[s];
        __syncthreads();
        for (int i = threadIdx.x; i < d; i += 256) xs[i] = sae_in[row * d + i];
        __syncthreads();
        for (int j = j_lo + wv; j < j_hi; j += 4) {
            const float* w = W_encT + (int64_t)j * d;
            float a = 0.f;
            for (int i = 4 * lane; i < d; i += 256) {
                const float4 wv4 = *reinterpret_cast<const float4*>(w + i);
                a = fmaf(xs[i], wv4.x, a); a = fmaf(xs[i + 1], wv4.y, a); a = fmaf(xs[i + 2], wv4.z, a); a = fmaf(xs[i + 3], wv4.w, a);
            }
            a = wave_sum(a);
            if (lane == 0) hidden[row * d_sae + j] = a + b_enc[j];
        }
    }
}
}  // namespace

int launch_enc_wmax(const float* enc_colsq, int d_sae, float* wmax, uint32_t* fb_count, uint32_t* feat_cnt, hipStream_t stream) {
    PV_REQUIRE(d_sae % 4 == 0 && ((uintptr_t)enc_colsq | (uintptr_t)feat_cnt) % 16 == 0, "enc_colsq / feat_cnt: 16-byte aligned, d_sae % 4 == 0");
    hipLaunchKernelGGL(sae_wmax_kernel, dim3(1), dim3(256), 0, stream, enc_colsq, d_sae, wmax, fb_count, feat_cnt);
    PV_LAUNCH_CHECK("sae_wmax_kernel");
    return PV_OK;
}

// debug: workgroups of the filtered encoder's small kernels the runtime says fit a CU (tools/probes/select_timeline.py counts six select
// workgroups alive per CU where the compiler's register model says eight)
extern "C" int pv_debug_select_occupancy(int32_t* out4) {
    int n = 0;
    PV_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, reinterpret_cast<const void*>(&sae_select_kernel<3, false>), 256, 0));
    out4[0] = n;
    PV_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, reinterpret_cast<const void*>(&sae_thr_kernel<32>), 256, 0));
    out4[1] = n;
    if (const int rc = relu_select_occupancy(&n)) return rc;
    out4[2] = n;
    hipFuncAttributes fa;
    PV_HIP_CHECK(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&sae_select_kernel<3, false>)));
    out4[3] = fa.numRegs;
    return PV_OK;
}

int sae_encode_fast(const pv_sae_desc& d, const pv_sae_state* st, int N, int32_t* topk_idx, float* topk_val,
                    uint32_t* feat_cnt, uint32_t* wpos, unsigned char* wsb, const SaeWs& ws, hipStream_t stream, const SaePre* pre) {
    PV_REQUIRE(st->W_encT && st->W_enc16T && st->enc_colsq, "encoder shadows (W_encT, W_enc16T, enc_colsq) are required");
    const int S = PV_SAE_SAMPLE_STRIDE, ns = d.d_sae / S, q = pv_sae_sample_q(d.k);
    float* wmax = (float*)(wsb + ws.wmax);
    uint32_t* fb_count = (uint32_t*)(wsb + ws.fb_count);
    int32_t* fb_list = (int32_t*)(wsb + ws.fb_list);
    int rc = pre ? PV_OK : launch_enc_wmax(st->enc_colsq, d.d_sae, wmax, fb_count, feat_cnt, stream);      // (the fused pre-pass: a workgroup of the prep launch did this)
    EncParams p = {};
    p.A = wsb + ws.x16; p.M = N; p.K = d.d_in; p.lda = d.d_in;
    // pass 0: every S-th feature
    p.B = st->W_enc16T; p.N = ns; p.ldb_bytes = (uint32_t)S * d.d_in * 2u; p.b_span = (uint32_t)ns * p.ldb_bytes;
    p.bias = st->b_enc; p.bias_stride = S; p.out = (float*)(wsb + ws.sample); p.ldo = ns;
    if (!rc) rc = launch_enc_gemm(0, p, stream);
    if (rc) return rc;
    const int nb_thr = (N + 3) / 4, nb_cf = (pre && !pre->have_mean) ? (d.d_in + 15) / 16 : 0;
    auto thr = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(nb_thr + nb_cf), dim3(256), 0, stream, (const float*)(wsb + ws.sample), ns,
                           (const float*)(wsb + ws.xnorm), (const float*)wmax, q, d.d_in, (float*)(wsb + ws.thr), (float*)(wsb + ws.sq),
                           (float*)(wsb + ws.band), N, nb_thr, (const float*)(wsb + ws.colpart), (float*)(wsb + ws.batch_mean),
                           (N + 15) / 16, 1.0f / (float)N);
    };
    if (ns <= 1024) thr(sae_thr_kernel<16>); else if (ns <= 2048) thr(sae_thr_kernel<32>); else thr(sae_thr_kernel<64>);      // d_sae <= 65536: ns <= 4096
    PV_LAUNCH_CHECK("sae_thr_kernel");
    // filter: all features
    p.N = d.d_sae; p.ldb_bytes = (uint32_t)d.d_in * 2u; p.b_span = (uint32_t)d.d_sae * p.ldb_bytes; p.bias_stride = 1;
    p.out = nullptr; p.thr = (const float*)(wsb + ws.thr); p.cnt = (uint32_t*)(wsb + ws.cand_cnt); p.cand = (int2*)(wsb + ws.cand);
#ifdef PV_ENC_TRACE
    p.trace = reinterpret_cast<uint64_t*>(wsb + ws.hidden) + 4 * 8192;      // (behind the select kernel's stamps)
#endif
    const int ntn = d.d_sae / 256;
    p.slots = pv_sae_tile_slots(d);
    rc = launch_enc_gemm(1, p, stream);
    if (rc) return rc;
    auto select = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(N), dim3(256), 0, stream, (const float*)(wsb + ws.sae_in), (const float*)st->W_encT,
                           (const float*)st->b_enc, (const uint32_t*)(wsb + ws.cand_cnt), (const int2*)(wsb + ws.cand),
                           (const float*)(wsb + ws.sq), (const float*)(wsb + ws.band), topk_idx, topk_val, fb_list, fb_count, feat_cnt, wpos,
                           d.d_in, d.k, ntn, p.slots, pre ? pre->x : (const float*)nullptr, (const float*)(wsb + ws.batch_mean),
                           (float*)(wsb + ws.norm), pre ? pre->d_true : 0, (float*)(wsb + ws.hidden));
    };
    const bool inline_fb = pre && g_pv_tuning.sae_inline_fb;
#define CALL(D)                                            \
    if (inline_fb) select(sae_select_kernel<D, true>);     \
    else select(sae_select_kernel<D, false>)
    V4_DISPATCH(d.d_in, CALL);
#undef CALL
    PV_LAUNCH_CHECK("sae_select_kernel");
    if (inline_fb) return PV_OK;                                // (undecided tokens were recomputed inside the select kernel)
    // undecided tokens: exact rows + the streaming / radix top-k (both launches are empty-handed when the list is empty)
    hipLaunchKernelGGL(sae_fb_hidden_kernel, dim3(PV_SAE_FB_SLOTS, (d.d_sae + 1023) / 1024), dim3(256), 0, stream,
                       (const float*)(wsb + ws.sae_in), (const float*)st->W_encT, (const float*)st->b_enc, (const int32_t*)fb_list,
                       (const uint32_t*)fb_count, (float*)(wsb + ws.hidden), d.d_in, d.d_sae);
    PV_LAUNCH_CHECK("sae_fb_hidden_kernel");
    sae_topk_rows((const float*)(wsb + ws.hidden), topk_idx, topk_val, d.d_sae, d.k, N, fb_list, fb_count, PV_SAE_FB_SLOTS, feat_cnt, wpos, stream);
    return PV_OK;
}
