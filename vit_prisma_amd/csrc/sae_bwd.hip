// The sparse backward of the k-sparse SAE steps (the data flow of a step: sae.hip), behind the step's decode kernel:
//   csr         active (token, slot) pairs grouped by feature: count -> scan -> fill, the lists put into token order
//   backward    per feature j: gW_dec[j,:] = sum a dY[n,:] ; gW_encT[j,:] = sum g sae_in[n,:] ; gb_enc[j] = sum g
//               (rows of both gradients are written coalesced; W_enc's gradient is kept TRANSPOSED, [d_sae][d_in])
// Callers: sae_sparse_tail (pv_sae_step, pv_sae_relu_step), sae_gated_sparse, pv_sae_gated_topk_step, pv_sae_tp_finish -- through
// sae_csr_build / sae_csr_grads / sae_csr_backward at the end of this file, which take a SaeBwd (sae_bwd.hpp).
#include "sae_bwd.hpp"

namespace {

// ------------------------------------------------------------------------------------------------
// CSR by feature of the active (token, slot) pairs
// ------------------------------------------------------------------------------------------------
// The pair counts per feature come out of the top-k selection (feat_cnt); csr_scan_kernel turns them into offsets,
// csr_fill_body scatters the pairs (no atomics), csr_post_body (a) cuts the CSR-ordered pair sequence into the chunks
// the short-list backward's waves own -- nominally BWD_CH pairs each, but a cut that would fall inside a list moves
// forward to that list's end, so a chunk is a run of WHOLE lists of which only the last can be long -- and (b) registers
// the features with more than BWD_LMAX pairs (dense features: on the bench batch 1.5 % of the features hold 36 % of the
// pairs) with their BWD_SEG-pair segments.  No gradient row is ever shared between waves, none needs atomics, every row is
// written exactly once.
// the token-range form sorts a list through a token-indexed LDS array: N tokens x 4 bytes (+ scratch) must fit the 160 KB
static inline bool sae_long_ranged(int n_tokens) { return (size_t)n_tokens * 4 + 4096 <= 150 * 1024; }

// single-workgroup exclusive scan over the d_sae counts, staged through LDS in blocks of 32768 features (one block for
// the 24 576-feature bench shape, two for the x64 SAEs of docs/sae_table.md: 49 152): coalesced load, per-thread contiguous
// runs scanned out of LDS, shuffles across threads, coalesced store, the running total carried into the next block
// loss_part (optional): this workgroup also reduces the decode kernel's per-token loss terms, scalars[0] = scalars[1] = loss_scale *
// their sum in a fixed order (the step's loss; it used to be a launch of its own in front of this one)
__global__ __launch_bounds__(1024) void csr_scan_kernel(const uint32_t* __restrict__ cnt, uint32_t* __restrict__ offs,
                                                        uint32_t* __restrict__ n_long, int d_sae,
                                                        float* __restrict__ scalars, float tokens,
                                                        const float* __restrict__ loss_part = nullptr, int n_loss = 0,
                                                        float loss_scale = 0.f) {
    constexpr int BLK = 32768;
    __shared__ uint32_t buf[BLK];
    __shared__ uint32_t wsum[16];
    __shared__ float lsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (loss_part) {
        float s = 0.f;
        for (int i = tid; i < n_loss; i += 1024) s += loss_part[i];
        s = wave_sum(s);
        if (lane == 0) lsum[wv] = s;
        __syncthreads();
        if (tid == 0) {
            float t = 0.f;
            for (int w = 0; w < 16; ++w) t += lsum[w];               // fixed order
            scalars[0] = t * loss_scale;
            scalars[1] = t * loss_scale;
        }
    }
    uint32_t carry = 0;
    for (int b0 = 0; b0 < d_sae; b0 += BLK) {
        const int nb = min(BLK, d_sae - b0);
        __syncthreads();                                 // (the previous block's stores out of buf, its reads of wsum)
        for (int i = tid; i < nb; i += 1024) buf[i] = cnt[b0 + i];
        __syncthreads();
        const int per = (nb + 1023) / 1024;
        const int lo = min(tid * per, nb), hi = min(lo + per, nb);
        uint32_t s = 0;
        for (int i = lo; i < hi; ++i) s += buf[i];
        uint32_t inc = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t a = __shfl_up(inc, o, 64);
            if (lane >= o) inc += a;
        }
        if (lane == 63) wsum[wv] = inc;
        __syncthreads();
        uint32_t base = carry;
        for (int w = 0; w < wv; ++w) base += wsum[w];
        uint32_t total = 0;
        for (int w = 0; w < 16; ++w) total += wsum[w];
        uint32_t run = base + inc - s;                  // exclusive prefix of this thread's run
        for (int i = lo; i < hi; ++i) {
            const uint32_t c = buf[i];
            buf[i] = run;
            run += c;
        }
        __syncthreads();
        for (int i = tid; i < nb; i += 1024) offs[b0 + i] = buf[i];
        carry += total;
    }
    if (tid == 1023) {
        offs[d_sae] = carry;
        if (scalars) scalars[2] = (float)carry / tokens;                // l0 = mean_n #(val > 0), train_sae.py:364 (divided, as in scan_body_256)
    }
    if (tid == 0) { n_long[0] = 0u; n_long[1] = 0u; n_long[2] = 0u; }   // counters of csr_post_body; the ticket of colsum_final_sq_kernel
}

// Per feature (one thread each), after the scan:
//   * firing statistics (train_sae.py:356-361);
//   * the chunk cuts of the short-list backward: the grid point g = w * BWD_CH that falls inside this feature's list
//     [beg, end) becomes chunk_start[w] = end (beg itself when g == beg) -- every grid point below the total lies in
//     exactly one list, so the scatter is disjoint; the cuts at and beyond the total are filled by the whole grid;
//   * long lists (> BWD_LMAX pairs): registered in long_list {feature, first segment, #segments} with their
//     BWD_SEG-pair segments in seg_range (two device counters, zeroed by the scan kernel).
struct CsrPostArgs {
    const uint32_t* offs; uint32_t* chunk_start; int max_chunks; int32_t* long_list; uint32_t* n_long; uint32_t* seg_range; int max_segs;
    float* act_freq; float* n_since_fired; float* fire_count; int d_sae; int update_stats; float* gb_enc_sparse; float* rowsq_sparse;
    int ranged; const uint32_t* gate;
};
// bid / nblocks: this workgroup's index among the nblocks that run the post pass (a block range of csr_post_fill_kernel)
__device__ __forceinline__ void csr_post_body(int bid, int nblocks, const uint32_t* __restrict__ offs, uint32_t* __restrict__ chunk_start,
                                                       int max_chunks, int32_t* __restrict__ long_list, uint32_t* __restrict__ n_long,
                                                       uint32_t* __restrict__ seg_range, int max_segs, float* __restrict__ act_freq,
                                                       float* __restrict__ n_since_fired, float* __restrict__ fire_count,
                                                       int d_sae, int update_stats, float* __restrict__ gb_enc_sparse,
                                                       float* __restrict__ rowsq_sparse, int ranged,
                                                       const uint32_t* __restrict__ gate) {
    if (gate && *gate != 0u) update_stats = 0;                    // (pv_sae_relu_step in dense mode: the dense path owns the statistics)
    const int j = bid * 256 + threadIdx.x;
    {   // the cuts at and beyond the total (all threads of the pass: a feature shard of the feature-parallel step keeps a
        // fraction of the N k pairs the cut array is sized for -- 7 of 8 cuts lie beyond the total at world 8)
        const uint32_t total = offs[d_sae];
        for (uint32_t w = (total + BWD_CH - 1) / BWD_CH + (uint32_t)j; w <= (uint32_t)max_chunks; w += (uint32_t)nblocks * 256u) chunk_start[w] = total;
    }
    if (j >= d_sae) return;
    const uint32_t beg = offs[j], end = offs[j + 1], c = end - beg;
    const float cnt = (float)c;
    if (fire_count) fire_count[j] = cnt;
    if (gb_enc_sparse && c == 0) {                    // PV_SAE_SPARSE_GRADS: the rows stay as they are, the scalars are zeroed here
        gb_enc_sparse[j] = 0.f;
        rowsq_sparse[j] = 0.f;
    }
    if (update_stats) {
        act_freq[j] += cnt;
        n_since_fired[j] = cnt > 0.f ? 0.f : n_since_fired[j] + 1.f;
    }
    for (uint32_t w = (beg + BWD_CH - 1) / BWD_CH; w * BWD_CH < end; ++w) chunk_start[w] = w * BWD_CH == beg ? beg : end;
    if (c > (uint32_t)BWD_LMAX) {
        const uint32_t e = atomicAdd(&n_long[0], 1u);
        long_list[3 * e] = j;
        if (ranged) return;                                       // (sae_long_sort_kernel cuts the list at the token ranges)
        const uint32_t nseg = (c + BWD_SEG - 1) / BWD_SEG;
        const uint32_t sb = atomicAdd(&n_long[1], nseg);
        long_list[3 * e + 1] = (int32_t)sb;
        long_list[3 * e + 2] = (int32_t)nseg;
        for (uint32_t sg = 0; sg < nseg && sb + sg < (uint32_t)max_segs; ++sg) {
            seg_range[2 * (sb + sg)] = beg + sg * BWD_SEG;
            seg_range[2 * (sb + sg) + 1] = min(beg + (sg + 1) * BWD_SEG, end);
        }
    }
}

__device__ __forceinline__ void csr_fill_body(int bid, const int32_t* __restrict__ idx, const uint32_t* __restrict__ wpos,
                                              const uint32_t* __restrict__ offs, int32_t* __restrict__ pairs, int n_pairs) {
    const int p = bid * 256 + threadIdx.x;
    if (p >= n_pairs) return;
    const uint32_t w = wpos[p];
    if (w != 0xffffffffu) pairs[offs[idx[p]] + w] = p;
}

// The three passes behind the scan that depend on nothing but it and the decode kernel, as ONE launch (they were three): blocks
// [0, nb_post) = csr_post, [nb_post, nb_post + nb_fill) = csr_fill, the rest (cs_x != NULL) = the 16-row partial column sums of dY
// that the bias gradients start from.
// nb_cs (the column-sum workgroups; 0: none) + one more workgroup when loss_part != NULL: the step's loss (loss_reduce_body: the scan ran as a
// role of the decode launch and could not take it)
__global__ __launch_bounds__(256) void csr_post_fill_kernel(const CsrPostArgs a, int nb_post, const int32_t* __restrict__ idx,
                                                            const uint32_t* __restrict__ wpos, int32_t* __restrict__ pairs, int n_pairs,
                                                            int nb_fill, const float* __restrict__ cs_x, float* __restrict__ cs_partial,
                                                            int cs_rows, int cs_d, int nb_cs, const float* __restrict__ loss_part = nullptr,
                                                            int n_loss = 0, float loss_scale = 0.f, float* __restrict__ scalars = nullptr) {
    const int b = blockIdx.x;
    if (b < nb_post)
        csr_post_body(b, nb_post, a.offs, a.chunk_start, a.max_chunks, a.long_list, a.n_long, a.seg_range, a.max_segs, a.act_freq,
                      a.n_since_fired, a.fire_count, a.d_sae, a.update_stats, a.gb_enc_sparse, a.rowsq_sparse, a.ranged, a.gate);
    else if (b < nb_post + nb_fill)
        csr_fill_body(b - nb_post, idx, wpos, a.offs, pairs, n_pairs);
    else if (b < nb_post + nb_fill + nb_cs)
        colsum_partial_body(b - nb_post - nb_fill, cs_x, cs_partial, cs_rows, cs_d);
    else
        loss_reduce_body(loss_part, n_loss, loss_scale, scalars);
}

// The position of a pair inside its feature's list was drawn by an integer atomic in the selection kernel: the SET of a list is
// exact, its ORDER is whatever the atomics produced -- and the backward sums in list order, so gradients would agree from run to run
// only up to fp32 summation order.  Short lists (<= BWD_LMAX = 64 pairs: one wave holds a whole list) are put into ascending pair
// order here (a pair id is token * k + slot and a feature holds a token at most once: token order) with a 64-lane bitonic network;
// the long lists get the same from sae_long_sort_kernel.  With both, every gradient is bit-reproducible.
__device__ __forceinline__ void csr_sort_short_body(int bid, const uint32_t* __restrict__ offs, int32_t* __restrict__ pairs, int d_sae) {
    const int lane = threadIdx.x & 63;
    const int f = bid * 4 + (threadIdx.x >> 6);
    if (f >= d_sae) return;
    const uint32_t o = offs[f];
    const int c = (int)(offs[f + 1] - o);
    if (c < 2 || c > BWD_LMAX) return;                        // (wave-uniform)
    int v = lane < c ? pairs[o + lane] : 0x7fffffff;
#pragma unroll
    for (int k2 = 2; k2 <= 64; k2 <<= 1)
#pragma unroll
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            const int other = __shfl_xor(v, j, 64);
            const bool up = (lane & k2) == 0, lower = (lane & j) == 0;
            v = (lower == up) ? min(v, other) : max(v, other);
        }
    if (lane < c) pairs[o + lane] = v;
}
__global__ __launch_bounds__(256) void csr_sort_short_kernel(const uint32_t* __restrict__ offs, int32_t* __restrict__ pairs, int d_sae) {
    csr_sort_short_body(blockIdx.x, offs, pairs, d_sae);
}

// ------------------------------------------------------------------------------------------------
// sparse backward:  gW_dec[j, :] = sum_p a_p dY[n_p, :],  gW_enc^T[j, :] = sum_p g_p sae_in[n_p, :],  gb_enc[j] = sum_p g_p
// over the pairs p = (token n_p, feature j) of feature j's list (a = kept activation, g = dh).  One-wave-per-feature
// collapses on skewed data (8.6 ms / step measured), so the work is split by PAIRS:
//   short lists (<= BWD_LMAX pairs)  sae_backward_kernel: wave w owns the chunk [chunk_start[w], chunk_start[w+1]) of whole
//                                    lists (~BWD_CH pairs), accumulates per feature and stores each finished row once
//   long lists                       cut into BWD_SEG-pair segments: sae_backward_seg_kernel (a wave per segment -> partial
//                                    rows in scratch), then sae_backward_long_kernel (a wave per dense feature sums its
//                                    segments in order, one store).  A feature that fires on all 4096 tokens is 128
//                                    independent waves, not one long chain
// Rows of features that did not fire are zeroed by the caller (this IS their zero_grad).  No atomics.
// Shared inner loop: the pair metadata of a run is fetched up front, one pair per lane, and broadcast with readlane, so the
// only memory operations inside the loop are the row gathers (16 bytes per lane), issued two pairs ahead of their use
// (vmcnt retires loads in order: nothing younger may sit between a gather and its use).
// ------------------------------------------------------------------------------------------------
template <int V4>
struct BwdAcc {
    float4 gd[V4], ge[V4];
    float gb;
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int i = 0; i < V4; ++i) { gd[i] = make_float4(0.f, 0.f, 0.f, 0.f); ge[i] = gd[i]; }
        gb = 0.f;
    }
    // the finished rows of feature j -> gW_dec[j], gW_encT[j], gb_enc[j]; rowsq[j] = their sum of squares (this feature's
    // term of the clip norm, so that the norm does not have to re-read the 151 MB it was just written to)
    __device__ __forceinline__ void store(int j, float* __restrict__ gW_dec, float* __restrict__ gW_encT, float* __restrict__ gb_enc,
                                          float* __restrict__ rowsq, int d, int lane, const int (&col)[V4], const bool (&ok)[V4]) const {
        float sq = 0.f;
#pragma unroll
        for (int i = 0; i < V4; ++i)
            if (ok[i]) {
                *reinterpret_cast<float4*>(gW_dec + (int64_t)j * d + col[i]) = gd[i];
                *reinterpret_cast<float4*>(gW_encT + (int64_t)j * d + col[i]) = ge[i];
                sq += gd[i].x * gd[i].x + gd[i].y * gd[i].y + gd[i].z * gd[i].z + gd[i].w * gd[i].w;
                sq += ge[i].x * ge[i].x + ge[i].y * ge[i].y + ge[i].z * ge[i].z + ge[i].w * ge[i].w;
            }
        sq = wave_sum(sq);
        if (lane == 0) {
            gb_enc[j] = gb;
            rowsq[j] = sq + gb * gb;
        }
    }
};

// accumulate the pairs [q0, q1) (all of ONE feature when STOP_AT_LONG is false).  With STOP_AT_LONG the run is a chunk of
// whole lists: a finished feature's rows are stored, and the walk ends at the first long list (the last list of a chunk).
// DUAL (the gated step, sae_gated_sparse): a pair carries a SECOND decoder term -- gW_dec[j] = sum_p a_p dY[n_p] + b_p dYb[n_p] (b =
// val_b: relu(gate_pre), dYb: the gradient of the reconstruction through the gate) -- gathered and accumulated alongside the first.
template <int V4, bool STOP_AT_LONG, bool DUAL = false>
__device__ __forceinline__ void bwd_walk(BwdAcc<V4>& acc, uint32_t q0, uint32_t q1, const uint32_t* __restrict__ offs,
                                         const int32_t* __restrict__ pairs, const int32_t* __restrict__ idx,
                                         const float* __restrict__ val, const float* __restrict__ dh, const float* __restrict__ dY,
                                         const float* __restrict__ sae_in, float* __restrict__ gW_dec, float* __restrict__ gW_encT,
                                         float* __restrict__ gb_enc, float* __restrict__ rowsq, int d, int k, int lane,
                                         const int (&col)[V4], const bool (&ok)[V4], const float* __restrict__ val_b = nullptr,
                                         const float* __restrict__ dYb = nullptr) {
    int cur = -1;
    auto store_rows = [&](int j) {
        acc.store(j, gW_dec, gW_encT, gb_enc, rowsq, d, lane, col, ok);
        acc.clear();
    };
    bool stop = false;
    for (uint32_t base = q0; base < q1 && !stop; base += 64) {
        const int cnt = (int)min(64u, q1 - base);
        int my_n = 0, my_j = 0;
        float my_a = 0.f, my_g = 0.f, my_b = 0.f;
        if (lane < cnt) {
            const int32_t p = pairs[base + lane];
            my_n = p / k;
            my_j = idx[p];
            my_a = val[p];
            my_g = dh[p];
            if constexpr (DUAL) my_b = val_b[p];
        }
        constexpr int VB = DUAL ? V4 : 1;
        float4 dy0[V4], si0[V4], dy1[V4], si1[V4], db0[VB], db1[VB];
        auto gather = [&](float4 (&dy)[V4], float4 (&si)[V4], float4 (&db)[VB], int t) {
            const int n = __shfl(my_n, t, 64);
#pragma unroll
            for (int i = 0; i < V4; ++i) {
                dy[i] = ld4(dY + (int64_t)n * d + col[i], ok[i]);
                si[i] = ld4(sae_in + (int64_t)n * d + col[i], ok[i]);
                if constexpr (DUAL) db[i] = ld4(dYb + (int64_t)n * d + col[i], ok[i]);
            }
        };
        auto accumulate = [&](const float4 (&dy)[V4], const float4 (&si)[V4], const float4 (&db)[VB], int t) {
            const float a = __shfl(my_a, t, 64), g = __shfl(my_g, t, 64);
            const float b = DUAL ? __shfl(my_b, t, 64) : 0.f;
            if constexpr (STOP_AT_LONG) {
                const int j = __shfl(my_j, t, 64);
                if (j != cur) {
                    if (cur >= 0) store_rows(cur);
                    cur = j;
                    stop = offs[j + 1] - offs[j] > (uint32_t)BWD_LMAX;       // (uniform) the long-list kernel owns it
                }
                if (stop) return;
            }
#pragma unroll
            for (int i = 0; i < V4; ++i) {
                acc.gd[i].x += a * dy[i].x; acc.gd[i].y += a * dy[i].y; acc.gd[i].z += a * dy[i].z; acc.gd[i].w += a * dy[i].w;
                acc.ge[i].x += g * si[i].x; acc.ge[i].y += g * si[i].y; acc.ge[i].z += g * si[i].z; acc.ge[i].w += g * si[i].w;
                if constexpr (DUAL) {
                    acc.gd[i].x += b * db[i].x; acc.gd[i].y += b * db[i].y; acc.gd[i].z += b * db[i].z; acc.gd[i].w += b * db[i].w;
                }
            }
            acc.gb += g;
        };
        gather(dy0, si0, db0, 0);
        if (cnt > 1) gather(dy1, si1, db1, 1);
        for (int t = 0; t < cnt && !stop; t += 2) {
            accumulate(dy0, si0, db0, t);
            if (t + 2 < cnt) gather(dy0, si0, db0, t + 2);
            if (t + 1 < cnt && !stop) {
                accumulate(dy1, si1, db1, t + 1);
                if (t + 3 < cnt) gather(dy1, si1, db1, t + 3);
            }
        }
    }
    if constexpr (STOP_AT_LONG) {
        if (!stop && cur >= 0) store_rows(cur);
    }
}

template <int V4, bool DUAL = false>
__global__ __launch_bounds__(256) void sae_backward_kernel(
    const uint32_t* __restrict__ offs, const uint32_t* __restrict__ chunk_start, const int32_t* __restrict__ pairs,
    const int32_t* __restrict__ idx, const float* __restrict__ val, const float* __restrict__ dh, const float* __restrict__ dY,
    const float* __restrict__ sae_in, float* __restrict__ gW_dec, float* __restrict__ gW_encT, float* __restrict__ gb_enc,
    float* __restrict__ rowsq, int d, int k, int n_chunks, const uint32_t* __restrict__ gate = nullptr,
    const float* __restrict__ val_b = nullptr, const float* __restrict__ dYb = nullptr) {
    const int lane = threadIdx.x & 63;
    const int wv = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wv >= n_chunks) return;
    if (gate && *gate != 0u) return;
    const uint32_t q0 = chunk_start[wv], q1 = chunk_start[wv + 1];
    if (q0 >= q1) return;
    bool ok[V4];
    int col[V4];
#pragma unroll
    for (int i = 0; i < V4; ++i) {
        col[i] = 4 * lane + 256 * i;
        ok[i] = col[i] < d;
    }
    BwdAcc<V4> acc;
    acc.clear();
    bwd_walk<V4, true, DUAL>(acc, q0, q1, offs, pairs, idx, val, dh, dY, sae_in, gW_dec, gW_encT, gb_enc, rowsq, d, k, lane, col, ok, val_b,
                             dYb);
}

// long lists, stage 0 (token-range form): sort every long list by token and cut it at the BWD_RANGES token-range boundaries.
// The 86 us / 608 MB of the count-cut segments were row gathers out of a 25 MB working set (dY + sae_in of 4096 tokens) that no
// XCD's 4 MB L2 holds: with the lists in token order, segment (feature e, range r) only touches the N / 8 tokens of range r, and
// the segment kernel gives range r to the workgroups of XCD r (3 MB of rows per L2).  A feature's pairs are DISTINCT tokens,
// so the sort is a scatter into a token-indexed LDS array + a compaction -- which also makes the summation order of these
// lists independent of the order the select kernel's atomics drew their positions in.  One workgroup per long feature.
// bid / nblocks: this workgroup's index among the nblocks that sort long lists (a launch of its own, or the leading block range of csr_sort_kernel)
__device__ __forceinline__ void sae_long_sort_body(int bid, int nblocks, int32_t* __restrict__ slot, int32_t* __restrict__ long_list,
                                                   uint32_t* __restrict__ n_long, const uint32_t* __restrict__ offs,
                                                   int32_t* __restrict__ pairs, uint32_t* __restrict__ seg_range, int k, int n_tok,
                                                   int max_segs) {
    __shared__ uint32_t wsum[4], bnd[BWD_RANGES + 1];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t nl = n_long[0];
    if (bid == 0 && tid == 0) n_long[1] = min(nl * BWD_RANGES, (uint32_t)max_segs);
    const int chunk = (n_tok + 255) / 256;
    const int rs = (n_tok + BWD_RANGES - 1) / BWD_RANGES;
    for (uint32_t e = bid; e < nl; e += nblocks) {
        const int j = long_list[3 * e];
        const uint32_t beg = offs[j], c = offs[j + 1] - beg;
        __syncthreads();
        for (int i = tid; i < n_tok; i += 256) slot[i] = -1;
        if (tid <= BWD_RANGES) bnd[tid] = tid == 0 ? 0u : c;
        __syncthreads();
        for (uint32_t i = tid; i < c; i += 256) {
            const int32_t p = pairs[beg + i];
            slot[p / k] = p;
        }
        __syncthreads();
        const int t0 = tid * chunk, t1 = min(t0 + chunk, n_tok);
        uint32_t cnt = 0;
        for (int t = t0; t < t1; ++t) cnt += slot[t] >= 0;
        uint32_t inc = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t a = __shfl_up(inc, o, 64);
            if (lane >= o) inc += a;
        }
        if (lane == 63) wsum[wv] = inc;
        __syncthreads();
        uint32_t base = inc - cnt;
        for (int w = 0; w < wv; ++w) base += wsum[w];
        uint32_t pos = base;
        for (int t = t0; t < t1; ++t) {
            if (t > 0 && t % rs == 0) bnd[t / rs] = pos;       // (first token of range t / rs: everything before it)
            const int32_t p = slot[t];
            if (p >= 0) pairs[beg + pos++] = p;
        }
        __syncthreads();
        if (tid < BWD_RANGES) {
            const uint32_t sg = e * BWD_RANGES + tid;
            if (sg < (uint32_t)max_segs) {
                seg_range[2 * sg] = beg + bnd[tid];
                seg_range[2 * sg + 1] = beg + bnd[tid + 1];
            }
        }
        if (tid == 0) {
            long_list[3 * e + 1] = (int32_t)(e * BWD_RANGES);
            long_list[3 * e + 2] = BWD_RANGES;
        }
    }
}
__global__ __launch_bounds__(256) void sae_long_sort_kernel(int32_t* __restrict__ long_list, uint32_t* __restrict__ n_long,
                                                            const uint32_t* __restrict__ offs, int32_t* __restrict__ pairs,
                                                            uint32_t* __restrict__ seg_range, int k, int n_tok, int max_segs) {
    extern __shared__ int32_t slot[];                      // [n_tok] token -> pair (or -1)
    sae_long_sort_body(blockIdx.x, gridDim.x, slot, long_list, n_long, offs, pairs, seg_range, k, n_tok, max_segs);
}
// Both list sorts as ONE launch (they touch disjoint lists): workgroups [0, nb_long) = the long lists (first: they are the longer jobs),
// the rest = the short lists, four features per workgroup.  The launch carries the long sort's LDS (4 bytes per token).
__global__ __launch_bounds__(256) void csr_sort_kernel(int nb_long, int32_t* __restrict__ long_list, uint32_t* __restrict__ n_long,
                                                       const uint32_t* __restrict__ offs, int32_t* __restrict__ pairs,
                                                       uint32_t* __restrict__ seg_range, int k, int n_tok, int max_segs, int d_sae) {
    extern __shared__ int32_t slot[];
    if ((int)blockIdx.x < nb_long) sae_long_sort_body(blockIdx.x, nb_long, slot, long_list, n_long, offs, pairs, seg_range, k, n_tok, max_segs);
    else csr_sort_short_body(blockIdx.x - nb_long, offs, pairs, d_sae);
}

// long lists, stage 1: one wave per segment -> partial rows in scratch  [segment][gd | ge][d] (+ gb).  Segments are BWD_SEG-pair
// cuts (ranged == 0) or the BWD_RANGES token ranges of a sorted list (ranged == 1: segment 8 e + r goes to a workgroup with
// blockIdx % 8 == r, i.e. to XCD r)
template <int V4, bool DUAL = false>
__global__ __launch_bounds__(512) void sae_backward_seg_kernel(
    const uint32_t* __restrict__ offs, const uint32_t* __restrict__ seg_range, const uint32_t* __restrict__ n_long,
    const int32_t* __restrict__ pairs, const int32_t* __restrict__ idx, const float* __restrict__ val,
    const float* __restrict__ dh, const float* __restrict__ dY, const float* __restrict__ sae_in, float* __restrict__ seg_rows,
    float* __restrict__ seg_b, int d, int k, int max_segs, int ranged, const uint32_t* __restrict__ gate = nullptr,
    const float* __restrict__ val_b = nullptr, const float* __restrict__ dYb = nullptr) {
    if (gate && *gate != 0u) return;                               // (uniform over the grid: no barrier is skipped by a part of a workgroup)
    constexpr int NW = 8;                                          // waves per workgroup (token-range form: 512 threads)
    __shared__ __attribute__((aligned(16))) float part[NW * 2 * 256 * V4];      // [wave][gd | ge][256 V4] (token-range form)
    __shared__ float part_b[NW];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t nseg = min(n_long[1], (uint32_t)max_segs);
    bool ok[V4];
    int col[V4];
#pragma unroll
    for (int i = 0; i < V4; ++i) {
        col[i] = 4 * lane + 256 * i;
        ok[i] = col[i] < d;
    }
    if (!ranged) {
        const uint32_t nw = blockDim.x >> 6;
        for (uint32_t sg = blockIdx.x * nw + wv; sg < nseg; sg += gridDim.x * nw) {
            BwdAcc<V4> acc;
            acc.clear();
            bwd_walk<V4, false, DUAL>(acc, seg_range[2 * sg], seg_range[2 * sg + 1], offs, pairs, idx, val, dh, dY, sae_in, nullptr, nullptr,
                                      nullptr, nullptr, d, k, lane, col, ok, val_b, dYb);
            float* o = seg_rows + (int64_t)sg * 2 * d;
#pragma unroll
            for (int i = 0; i < V4; ++i)
                if (ok[i]) {
                    *reinterpret_cast<float4*>(o + col[i]) = acc.gd[i];
                    *reinterpret_cast<float4*>(o + d + col[i]) = acc.ge[i];
                }
            if (lane == 0) seg_b[sg] = acc.gb;
        }
        return;
    }
    // token-range form: the WORKGROUP owns segment (long feature e, range r = blockIdx % 8 = its XCD); its eight waves take an
    // eighth of the segment's (token-sorted) pairs each -- a dense feature has N / 8 pairs per range, one wave alone would be
    // the kernel's tail -- and their partial rows are summed in wave order through LDS
    constexpr int DP = 256 * V4;                                  // padded row length (floats)
    float* pw = part;
    for (uint32_t e = blockIdx.x >> 3; e * BWD_RANGES < nseg; e += gridDim.x >> 3) {
        const uint32_t sg = e * BWD_RANGES + (blockIdx.x & 7);
        const uint32_t q0 = seg_range[2 * sg], q1 = seg_range[2 * sg + 1];
        const uint32_t per = (q1 - q0 + NW - 1) / NW;
        const uint32_t w0 = min(q0 + wv * per, q1), w1 = min(w0 + per, q1);
        BwdAcc<V4> acc;
        acc.clear();
        bwd_walk<V4, false, DUAL>(acc, w0, w1, offs, pairs, idx, val, dh, dY, sae_in, nullptr, nullptr, nullptr, nullptr, d, k, lane, col, ok,
                                  val_b, dYb);
        __syncthreads();                                          // (the previous segment's reads of part)
#pragma unroll
        for (int i = 0; i < V4; ++i) {
            *reinterpret_cast<float4*>(pw + (wv * 2 + 0) * DP + col[i]) = acc.gd[i];
            *reinterpret_cast<float4*>(pw + (wv * 2 + 1) * DP + col[i]) = acc.ge[i];
        }
        if (lane == 0) part_b[wv] = acc.gb;
        __syncthreads();
        // 2 x d floats out: thread t sums column group t (gd for t < 64 V4 ... ) in wave order
        float* o = seg_rows + (int64_t)sg * 2 * d;
        for (int c4 = threadIdx.x; c4 < 2 * 64 * V4; c4 += NW * 64) {
            const int which = c4 / (64 * V4), cc = (c4 - which * 64 * V4) * 4;
            if (cc < d) {
                float4 t = *reinterpret_cast<const float4*>(pw + (0 * 2 + which) * DP + cc);
#pragma unroll
                for (int w = 1; w < NW; ++w) {
                    const float4 u = *reinterpret_cast<const float4*>(pw + (w * 2 + which) * DP + cc);
                    t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
                }
                *reinterpret_cast<float4*>(o + which * d + cc) = t;
            }
        }
        if (threadIdx.x == 0) {
            float t = part_b[0];
#pragma unroll
            for (int w = 1; w < NW; ++w) t += part_b[w];
            seg_b[sg] = t;
        }
    }
}

// long lists, stage 2: one wave per dense feature sums its segments' partial rows in segment order and stores
template <int V4>
__global__ __launch_bounds__(256) void sae_backward_long_kernel(
    const int32_t* __restrict__ long_list, const uint32_t* __restrict__ n_long, const float* __restrict__ seg_rows,
    const float* __restrict__ seg_b, float* __restrict__ gW_dec, float* __restrict__ gW_encT, float* __restrict__ gb_enc,
    float* __restrict__ rowsq, int d, int max_segs, const uint32_t* __restrict__ gate = nullptr) {
    if (gate && *gate != 0u) return;
    const int lane = threadIdx.x & 63;
    const uint32_t nl = n_long[0];
    bool ok[V4];
    int col[V4];
#pragma unroll
    for (int i = 0; i < V4; ++i) {
        col[i] = 4 * lane + 256 * i;
        ok[i] = col[i] < d;
    }
    for (uint32_t f = blockIdx.x * 4 + (threadIdx.x >> 6); f < nl; f += gridDim.x * 4) {
        const int j = long_list[3 * f];
        const uint32_t sb = (uint32_t)long_list[3 * f + 1], ns = (uint32_t)long_list[3 * f + 2];
        BwdAcc<V4> acc;
        acc.clear();
        const uint32_t s_end = min(sb + ns, (uint32_t)max_segs);
        for (uint32_t sg = sb; sg < s_end; sg += 4) {                 // four partial rows in flight, summed in segment order
            float4 a[4][V4], b[4][V4];
            float gb4[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool live = sg + u < s_end;
                const float* o = seg_rows + (int64_t)(live ? sg + u : sg) * 2 * d;
#pragma unroll
                for (int i = 0; i < V4; ++i) {
                    a[u][i] = ld4(o + col[i], ok[i] && live);
                    b[u][i] = ld4(o + d + col[i], ok[i] && live);
                }
                gb4[u] = live ? seg_b[sg + u] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
                for (int i = 0; i < V4; ++i) {
                    acc.gd[i].x += a[u][i].x; acc.gd[i].y += a[u][i].y; acc.gd[i].z += a[u][i].z; acc.gd[i].w += a[u][i].w;
                    acc.ge[i].x += b[u][i].x; acc.ge[i].y += b[u][i].y; acc.ge[i].z += b[u][i].z; acc.ge[i].w += b[u][i].w;
                }
                acc.gb += gb4[u];
            }
        }
        acc.store(j, gW_dec, gW_encT, gb_enc, rowsq, d, lane, col, ok);
    }
}

// The features no token kept: their gradient rows are zero (this IS their zero_grad).  One wave per feature; the others
// leave at once (their rows are stored, exactly once, by the backward kernels).
template <int V4>
__global__ __launch_bounds__(256) void sae_zero_empty_kernel(const uint32_t* __restrict__ offs, float* __restrict__ gW_dec,
                                                             float* __restrict__ gW_encT, float* __restrict__ gb_enc,
                                                             float* __restrict__ rowsq, int d_sae, int d,
                                                             const uint32_t* __restrict__ gate = nullptr) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gate && *gate != 0u) return;
    if (j >= d_sae || offs[j + 1] != offs[j]) return;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < V4; ++i) {
        const int c = 4 * lane + 256 * i;
        if (c < d) {
            *reinterpret_cast<float4*>(gW_dec + (int64_t)j * d + c) = z;
            *reinterpret_cast<float4*>(gW_encT + (int64_t)j * d + c) = z;
        }
    }
    if (lane == 0) {
        gb_enc[j] = 0.f;
        rowsq[j] = 0.f;
    }
}

int launch_long_sort(int32_t* long_list, uint32_t* n_long, const uint32_t* offs, int32_t* pairs, uint32_t* seg_range, int k, int N,
                     int max_segs, hipStream_t stream) {
    static bool attr_done = false;
    if (!attr_done) {
        PV_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&sae_long_sort_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         150 * 1024));
        attr_done = true;
    }
    hipLaunchKernelGGL(sae_long_sort_kernel, dim3(512), dim3(256), (size_t)N * 4, stream, long_list, n_long, offs, pairs, seg_range, k, N,
                       max_segs);
    PV_LAUNCH_CHECK("sae_long_sort_kernel");
    return PV_OK;
}
int launch_csr_sort(int32_t* long_list, uint32_t* n_long, const uint32_t* offs, int32_t* pairs, uint32_t* seg_range, int k, int N,
                    int max_segs, int d_sae, hipStream_t stream) {
    static bool attr_done = false;
    if (!attr_done) {
        PV_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&csr_sort_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         150 * 1024));
        attr_done = true;
    }
    const int nb_long = 512;
    hipLaunchKernelGGL(csr_sort_kernel, dim3(nb_long + (d_sae + 3) / 4), dim3(256), (size_t)N * 4, stream, nb_long, long_list, n_long, offs,
                       pairs, seg_range, k, N, max_segs, d_sae);
    PV_LAUNCH_CHECK("csr_sort_kernel");
    return PV_OK;
}

// The gradient launches of sae_csr_grads for one row width; DUAL: with the pairs' second decoder term (b.val_b, b.dY_b).
// Every gradient row is stored exactly once: by the zero kernel (features no token kept), the short-list kernel or the long-list
// combine.  b.sparse_grads: the rows of features no token kept are not touched at all -- pv_sae_apply takes their gradient as zero
// from the feature offsets this step leaves in the workspace (about half of the features on a trained-like batch: 2 x 39 MB not
// written here and not read there)
template <int V4, bool DUAL>
void launch_grads(const pv_sae_desc& d, pv_sae_state* st, const SaeBwd& b, unsigned char* wsb, const SaeWs& ws, hipStream_t stream) {
    const SaeTail& tb = b.tail;
    const uint32_t* offs = (const uint32_t*)(wsb + ws.offs);
    const int32_t* long_list = (const int32_t*)(wsb + ws.long_list);
    const uint32_t* n_long = (const uint32_t*)(wsb + ws.n_long);
    float* rowsq = (float*)(wsb + ws.rowsq);
    const int max_chunks = (b.N * b.k + BWD_CH - 1) / BWD_CH;
    const int ranged = sae_long_ranged(b.N) ? 1 : 0;
    const dim3 block(256);
    if (!b.sparse_grads)
        hipLaunchKernelGGL((sae_zero_empty_kernel<V4>), dim3((d.d_sae + 3) / 4), block, 0, stream, offs, st->gW_dec, st->gW_enc, st->gb_enc,
                           rowsq, d.d_sae, d.d_in, b.gate);
    hipLaunchKernelGGL((sae_backward_kernel<V4, DUAL>), dim3((max_chunks + 3) / 4), block, 0, stream, offs, (const uint32_t*)tb.chunk_start,
                       (const int32_t*)tb.pairs, b.idx, b.val, (const float*)tb.dh, b.dY, b.sae_in, st->gW_dec, st->gW_enc, st->gb_enc,
                       rowsq, d.d_in, b.k, max_chunks, b.gate, b.val_b, b.dY_b);
    hipLaunchKernelGGL((sae_backward_seg_kernel<V4, DUAL>), dim3(ranged ? 2048 : 1024), dim3(ranged ? 512 : 256), 0, stream, offs,
                       (const uint32_t*)tb.seg_range, n_long, (const int32_t*)tb.pairs, b.idx, b.val, (const float*)tb.dh, b.dY, b.sae_in,
                       tb.seg_rows, tb.seg_b, d.d_in, b.k, tb.max_segs, ranged, b.gate, b.val_b, b.dY_b);
    hipLaunchKernelGGL((sae_backward_long_kernel<V4>), dim3(256), block, 0, stream, long_list, n_long, (const float*)tb.seg_rows,
                       (const float*)tb.seg_b, st->gW_dec, st->gW_enc, st->gb_enc, rowsq, d.d_in, tb.max_segs, b.gate);
}

}  // namespace

int sae_csr_build(pv_sae_plan* plan, pv_sae_state* st, const SaeBwd& b, unsigned char* wsb, const SaeWs& ws, hipStream_t stream) {
    const pv_sae_desc& d = plan->d;
    const SaeTail& tb = b.tail;
    const int N = b.N, n_pairs = N * b.k;
    // CSR by feature: counts and within-list positions came out of the top-k selection; scan + atomic-free scatter
    const uint32_t* cnt = b.cnt ? b.cnt : (const uint32_t*)(wsb + ws.cnt);
    uint32_t* offs = (uint32_t*)(wsb + ws.offs);
    int32_t* long_list = (int32_t*)(wsb + ws.long_list);
    uint32_t* n_long = (uint32_t*)(wsb + ws.n_long);
    float* rowsq = (float*)(wsb + ws.rowsq);
    const int ranged = sae_long_ranged(N) ? 1 : 0;
    // (the scan's workgroup also reduces the loss: loss = mse_loss = sum / (N_global * d_in), sae.py:148; topk: loss == mse_loss,
    // :620-626 -- scalars[0] = scalars[1])
    if (!b.folded)
        hipLaunchKernelGGL(csr_scan_kernel, dim3(1), dim3(1024), 0, stream, cnt, offs, n_long, d.d_sae, b.scalars, (float)N, b.loss_part,
                           b.loss_part ? N : 0, b.loss_scale);
    // chunk cuts / long lists / statistics, the scatter of the pairs and (autoencoder) the partial column sums of dY: one launch
    {
        CsrPostArgs pa;
        pa.offs = offs; pa.chunk_start = tb.chunk_start; pa.max_chunks = (n_pairs + BWD_CH - 1) / BWD_CH; pa.long_list = long_list;
        pa.n_long = n_long; pa.seg_range = tb.seg_range; pa.max_segs = tb.max_segs; pa.act_freq = st->act_freq_scores;
        pa.n_since_fired = st->n_fwd_since_fired; pa.fire_count = b.fire_count; pa.d_sae = d.d_sae; pa.update_stats = b.update_stats;
        pa.gb_enc_sparse = b.sparse_grads ? st->gb_enc : nullptr; pa.rowsq_sparse = b.sparse_grads ? rowsq : nullptr; pa.ranged = ranged;
        pa.gate = b.gate;
        const int nb_post = (d.d_sae + 255) / 256, nb_fill = (n_pairs + 255) / 256, nb_cs = b.colsum_dY ? (N + CS_ROWS - 1) / CS_ROWS : 0;
        const int nb_loss = (b.folded && b.loss_part) ? 1 : 0;
        hipLaunchKernelGGL(csr_post_fill_kernel, dim3(nb_post + nb_fill + nb_cs + nb_loss), dim3(256), 0, stream, pa, nb_post, b.idx,
                           (const uint32_t*)tb.wpos, tb.pairs, n_pairs, nb_fill, b.dY, (float*)(wsb + ws.colpart), N, d.d_in, nb_cs,
                           nb_loss ? b.loss_part : (const float*)nullptr, N, b.loss_scale, b.scalars);
    }
    if (b.folded && ranged)
        return launch_csr_sort(long_list, n_long, (const uint32_t*)offs, tb.pairs, tb.seg_range, b.k, N, tb.max_segs, d.d_sae, stream);
    hipLaunchKernelGGL(csr_sort_short_kernel, dim3((d.d_sae + 3) / 4), dim3(256), 0, stream, (const uint32_t*)offs, tb.pairs, d.d_sae);
    if (ranged) {
        const int rc = launch_long_sort(long_list, n_long, (const uint32_t*)offs, tb.pairs, tb.seg_range, b.k, N, tb.max_segs, stream);
        if (rc) return rc;
    }
    PV_LAUNCH_CHECK("csr kernels");
    return PV_OK;
}

int sae_csr_grads(pv_sae_plan* plan, pv_sae_state* st, const SaeBwd& b, unsigned char* wsb, const SaeWs& ws, hipStream_t stream) {
    const pv_sae_desc& d = plan->d;
    plan->live_offs = b.sparse_grads ? (const uint32_t*)(wsb + ws.offs) : nullptr;
#define CALL(D)                                                   \
    if (b.val_b) launch_grads<D, true>(d, st, b, wsb, ws, stream); \
    else launch_grads<D, false>(d, st, b, wsb, ws, stream)
    V4_DISPATCH(d.d_in, CALL);
#undef CALL
    PV_LAUNCH_CHECK("sae_backward_kernel");
    return PV_OK;
}

int sae_csr_backward(pv_sae_plan* plan, pv_sae_state* st, const SaeBwd& b, unsigned char* wsb, const SaeWs& ws, hipStream_t stream) {
    const int rc = sae_csr_build(plan, st, b, wsb, ws, stream);
    if (rc) return rc;
    return sae_csr_grads(plan, st, b, wsb, ws, stream);
}
