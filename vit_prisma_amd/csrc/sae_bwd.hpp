// The sparse backward of the k-sparse SAE steps (sae_bwd.hip): the CSR by feature of the kept (token, slot) pairs and the gradient
// kernels behind it, and the decode launch in front of it (sae_decode, sae.hip).  Here: what their callers (sae.hip, sae_tp.hip,
// sae_gated_topk.hip, sae_dense.hip, sae_gated.hip) fill in (SaeDecode, SaeBwd), the sizes the workspace carvers need, and the device
// bodies that kernels of sae.hip, sae_bwd.hip, sae_apply.hip, sae_gated.hip and sae_gated_topk.hip share.
#pragma once
#include "sae.hpp"

// pairs per chunk of the short-list backward, the longest short list, pairs per count-cut segment of a long list (sae_bwd.hip)
constexpr int BWD_CH = 16;
constexpr int BWD_LMAX = 64;
constexpr int BWD_SEG = 32;
constexpr int BWD_RANGES = 8;               // token ranges of the long-list backward = XCDs (one L2 each)
// segments of the long lists: ceil(c / SEG) per list with c > LMAX pairs (count-cut form), or BWD_RANGES per list (token-range
// form; at most n_pairs / (LMAX + 1) long lists)
static inline size_t sae_max_segs(size_t n_pairs) {
    const size_t a = n_pairs / BWD_SEG + n_pairs / BWD_LMAX + 1, b = (size_t)BWD_RANGES * (n_pairs / (BWD_LMAX + 1) + 1);
    return a > b ? a : b;
}
constexpr int CS_ROWS = 16;                 // rows per workgroup of the column sums' first stage (colsum_partial_body)

// The k-dependent buffers (SaeTail) where the plan's workspace holds them, for a step of n_pairs = tokens x slots pairs ...
static inline SaeTail sae_tail(unsigned char* wsb, const SaeWs& ws, size_t n_pairs) {
    SaeTail tb;
    tb.dh = (float*)(wsb + ws.dh); tb.chunk_start = (uint32_t*)(wsb + ws.cursor); tb.wpos = (uint32_t*)(wsb + ws.wpos);
    tb.seg_range = (uint32_t*)(wsb + ws.seg_range); tb.seg_rows = (float*)(wsb + ws.seg_rows); tb.seg_b = (float*)(wsb + ws.seg_b);
    tb.pairs = (int32_t*)(wsb + ws.pairs); tb.max_segs = (int)sae_max_segs(n_pairs);
    return tb;
}
// ... and where the workspace of the ReLU / gated sparse forms (relu_carve) holds them
static inline SaeTail relu_tail(unsigned char* rwb, const ReluWs& rw) {
    SaeTail tb;
    tb.dh = (float*)(rwb + rw.dh); tb.chunk_start = (uint32_t*)(rwb + rw.cursor); tb.wpos = (uint32_t*)(rwb + rw.wpos);
    tb.seg_range = (uint32_t*)(rwb + rw.seg_range); tb.seg_rows = (float*)(rwb + rw.seg_rows); tb.seg_b = (float*)(rwb + rw.seg_b);
    tb.pairs = (int32_t*)(rwb + rw.pairs); tb.max_segs = rw.max_segs;
    return tb;
}

// The backward of a k-sparse step behind its decode kernel: the CSR by feature (counts and within-list positions came out of the
// selection), then the backward kernels -- every row of gW_dec / gW_enc^T / gb_enc written exactly once.  A caller sets the fields it means.
struct SaeBwd {
    int N = 0, k = 0;                        // N tokens of k slots: idx / val / tail.dh hold N k entries, dY / sae_in N rows
    const int32_t* idx = nullptr;            // the kept features ...
    const float* val = nullptr;              // ... and activations (<= 0: a hole); tail.dh: the gradient at them
    const float* dY = nullptr;
    const float* sae_in = nullptr;
    float* scalars = nullptr;                // [2] = l0 (the scan); [0] = [1] = the loss with loss_part
    SaeTail tail = {};                       // sae_tail / relu_tail
    float* fire_count = nullptr;             // optional: pairs per feature, as floats
    int update_stats = 0;                    // the firing statistics of st (train_sae.py:356-361)
    bool sparse_grads = false;               // PV_SAE_SPARSE_GRADS: rows of features no token kept stay unwritten (pv_sae_plan.live_offs)
    const float* loss_part = nullptr;        // optional: the decode kernel's N per-token loss terms, scalars[0] = scalars[1] = loss_scale * sum
    float loss_scale = 0.f;
    bool colsum_dY = false;                  // also the 16-row partial column sums of dY (ws.colpart) that the bias gradients start from
    const uint32_t* gate = nullptr;          // pv_sae_relu_step / the gated step: the mode word -- nonzero = the dense form runs, the kernels leave at once
    const uint32_t* cnt = nullptr;           // pair counts per feature that are not the selection's own (default: ws.cnt)
    const float* val_b = nullptr;            // the second decoder term of a pair (bwd_walk<DUAL>, the gated step): gW_dec[j] += sum val_b dY_b[n]
    const float* dY_b = nullptr;
    bool folded = false;                     // the scan has run as a role of the decode launch (ScanRole): the loss rides in the post + fill
                                             // launch, the two list sorts are one launch -- two launches in sae_csr_build instead of four
};
// The two halves of sae_csr_backward.  sae_csr_build: the CSR by feature -- scan, chunk cuts / long lists / statistics / pair scatter, the
// two list sorts; it reads the selection's output only (counts, positions, indices), so with loss_part == NULL and colsum_dY false it
// does not wait for the decode kernel.  sae_csr_grads: the backward kernels.
int sae_csr_build(pv_sae_plan* plan, pv_sae_state* st, const SaeBwd& b, unsigned char* wsb, const SaeWs& ws, hipStream_t stream);
int sae_csr_grads(pv_sae_plan* plan, pv_sae_state* st, const SaeBwd& b, unsigned char* wsb, const SaeWs& ws, hipStream_t stream);
int sae_csr_backward(pv_sae_plan* plan, pv_sae_state* st, const SaeBwd& b, unsigned char* wsb, const SaeWs& ws, hipStream_t stream);

// Device bodies shared across the file boundary.  In an anonymous namespace like the kernels of both files: ScanRole is a parameter of
// sae_decode_kernel, whose mangled name the profiles refer to.
#ifdef __HIPCC__
namespace {

// a lane's 16-byte column group of a row (zeros beyond the row's end)
__device__ __forceinline__ float4 ld4(const float* p, bool ok) {
    return ok ? *reinterpret_cast<const float4*>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
}
__device__ __forceinline__ float dot4(const float4& a, const float4& b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// column sums of a [rows][d] fp32 matrix (deterministic two-stage reduction).
// stage 1: partial[blk][c] over CS_ROWS-row blocks -- rows / 16 workgroups (256 at N = 4096: every CU busy), 16
// independent loads in flight per thread
__device__ __forceinline__ void colsum_partial_body(int bid, const float* __restrict__ x, float* __restrict__ partial, int rows, int d) {
    const int r0 = bid * CS_ROWS;
    for (int c = threadIdx.x; c < d; c += 256) {
        float v[CS_ROWS];
#pragma unroll
        for (int i = 0; i < CS_ROWS; ++i) v[i] = (r0 + i < rows) ? x[(int64_t)(r0 + i) * d + c] : 0.f;
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < CS_ROWS; ++i) s += v[i];          // fixed order
        partial[(int64_t)bid * d + c] = s;
    }
}

// The exclusive scan of csr_scan_kernel as ONE 256-thread workgroup without its LDS staging (a role of the decode launch, see
// sae_decode_kernel: the scan reads the selection's counts only, so it does not have to wait for the decode kernel -- it runs inside it):
// every thread owns a contiguous run of counts, sums it with 16-byte loads, the runs are scanned by shuffles, the offsets are written
// in a second walk over the (cached) counts.  Integer arithmetic: the offsets are csr_scan_kernel's.  Also its other duties: the
// total (offs[d_sae], scalars[2] = l0) and the zeroing of the long-list counters.  The loss reduction that rides in csr_scan_kernel's
// workgroup cannot come along (it needs the decode kernel's output): loss_reduce_body, a role of csr_post_fill_kernel.
struct ScanRole {
    const uint32_t* cnt; uint32_t* offs; uint32_t* n_long; int d_sae; float* scalars; float tokens;
};
__device__ __forceinline__ void scan_body_256(const ScanRole& r) {
    __shared__ uint32_t sc_wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int per = (((r.d_sae + 255) / 256) + 3) & ~3;
    const int lo = min(tid * per, r.d_sae), hi = min(lo + per, r.d_sae);
    const bool quads = (r.d_sae & 3) == 0;                   // (then lo and hi are multiples of four)
    uint32_t s = 0;
    {
        int i = lo;
        if (quads) {
#pragma unroll 8
            for (; i + 4 <= hi; i += 4) {
                const uint4 c = *reinterpret_cast<const uint4*>(r.cnt + i);
                s += c.x + c.y + c.z + c.w;
            }
        }
        for (; i < hi; ++i) s += r.cnt[i];
    }
    uint32_t inc = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t a = __shfl_up(inc, o, 64);
        if (lane >= o) inc += a;
    }
    if (lane == 63) sc_wsum[wv] = inc;
    __syncthreads();
    uint32_t base = 0, total = 0;
    for (int w = 0; w < 4; ++w) {
        base += w < wv ? sc_wsum[w] : 0u;
        total += sc_wsum[w];
    }
    uint32_t run = base + inc - s;                           // exclusive prefix of this thread's run
    {
        int i = lo;
        if (quads)
#pragma unroll 8
            for (; i + 4 <= hi; i += 4) {
                const uint4 c = *reinterpret_cast<const uint4*>(r.cnt + i);
                uint4 o;
                o.x = run; o.y = run + c.x; o.z = o.y + c.y; o.w = o.z + c.z;
                run = o.w + c.w;
                *reinterpret_cast<uint4*>(r.offs + i) = o;
            }
        for (; i < hi; ++i) {
            const uint32_t c = r.cnt[i];
            r.offs[i] = run;
            run += c;
        }
    }
    if (tid == 255) {
        r.offs[r.d_sae] = total;
        if (r.scalars) r.scalars[2] = (float)total / r.tokens;          // l0 = mean_n #(val > 0), train_sae.py:364 (a division: total * (1 / N)
                                                                        // is an ulp off at some N -- 1328 pairs of 166 tokens gave 7.9999995)
    }
    if (tid == 0) { r.n_long[0] = 0u; r.n_long[1] = 0u; r.n_long[2] = 0u; }      // counters of csr_post_body; the ticket of colsum_final_sq_kernel
}

// The step's loss from the decode kernel's per-token terms: scalars[0] = scalars[1] = loss_scale * sum, in the order of the 1024-thread
// reduction that rides in csr_scan_kernel's workgroup (thread t of 1024 takes terms t, t + 1024, ...; 16 wave sums; added in wave
// order) -- here by 256 threads that each play four of those threads, so that the two homes of the reduction agree to the bit.
__device__ __forceinline__ void loss_reduce_body(const float* __restrict__ loss_part, int n_loss, float loss_scale, float* __restrict__ scalars) {
    __shared__ float lsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float t = 0.f;
        for (int i = tid + 256 * q; i < n_loss; i += 1024) t += loss_part[i];
        t = wave_sum(t);
        if (lane == 0) lsum[wv + 4 * q] = t;
    }
    __syncthreads();
    if (tid == 0) {
        float t = 0.f;
        for (int w = 0; w < 16; ++w) t += lsum[w];               // fixed order
        scalars[0] = t * loss_scale;
        scalars[1] = t * loss_scale;
    }
}

// the scan as a role of a decode launch over the pair counts cnt of N tokens: offsets -> ws.offs, scalars[2] = l0
static inline ScanRole sae_scan_role(const pv_sae_desc& d, unsigned char* wsb, const SaeWs& ws, const uint32_t* cnt, float* scalars, int N) {
    return ScanRole{cnt, (uint32_t*)(wsb + ws.offs), (uint32_t*)(wsb + ws.n_long), d.d_sae, scalars, (float)N};
}

}  // namespace

// One launch of sae_decode_kernel (sae.hip): decode + LN-out + loss terms + dY + dh of N tokens of k slots, one wave per token.  A
// caller sets the fields it means.
struct SaeDecode {
    int mode = 0;                            // 0: the whole thing; the feature-parallel step cuts it at the reconstruction -- 1: this rank's
                                             // partial sum_s val_s W_dec[idx_s] only, written to sae_out (no b_dec, no LN-out); 2: everything
                                             // behind it
    int N = 0, d = 0, k = 0;                 // tokens, d_in, slots per token (pv_sae_relu_step: the per-token capacity)
    const float* x = nullptr;                // what the loss is taken against (a transcoder, pv_sae_state.tc: the TARGET)
    const float* W_dec = nullptr;
    const float* b_dec = nullptr;            // (a transcoder: b_dec_out)
    const int32_t* idx = nullptr;            // the kept features ...
    const float* val = nullptr;              // ... and activations; <= 0: a hole (no gather, dh = 0)
    const float* mu = nullptr;               // LN-out: out = (reconstruction + b_dec) * sd + mu
    const float* sd = nullptr;
    const float* norm = nullptr;             // the loss normaliser ||x_n - mean_batch(x)||_2
    float* sae_out = nullptr;                // optional (mode 1: the partial sums)
    float* dY = nullptr;                     // with dh, the gradients; NULL: none are wanted (inference)
    float* dh = nullptr;                     // [N k] the gradient at the kept activations
    float* loss_part = nullptr;              // [N] per-token loss terms
    float grad_scale = 0.f;                  // 2 / (N_global * d_in)
    const float* inv_norm = nullptr;         // set_decoder_norm_to_unit_norm is pending: W_dec still holds the un-normalised rows and row j
                                             // stands for W_dec[j] * inv_norm[j] (the Adam kernel writes the normalised + updated row; see
                                             // pv_sae_step)
    const float* pre_sum = nullptr;          // mode 2: [N, d_in] the reconstruction summed over the ranks (without b_dec)
    const float* addend = nullptr;           // mode 0, a transcoder: the skip term x_in @ W_skip^T the reconstruction starts from
    float dh_add = 0.f;                      // pv_sae_relu_step: l1_coefficient / N_global, the L1 term's gradient on every kept activation
                                             // (sae.py:617-626)
    const uint32_t* tok_cnt = nullptr;       // pv_sae_relu_step: tok_cnt[n] = the pairs token n holds (front-packed; the rest of the row are holes)
    const uint32_t* gate = nullptr;          // pv_sae_relu_step: the step's mode word -- nonzero = the step runs on the dense GEMMs, leave at once
    ScanRole scan = {};                      // sae_scan_role: the launch carries one more workgroup, which runs the CSR scan (modes 0 and 2)
};
int sae_decode(const SaeDecode& a, hipStream_t stream);
#endif
