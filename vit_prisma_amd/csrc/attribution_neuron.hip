// Direct logit attribution by MLP neuron on the cached mlp.hook_post taps (gfx950): the dense form and a streaming exact top-k.
//
// Reference semantics (activation_cache.py:523-654, :656-735): get_neuron_results materialises r = post[..., n, None] * W_out[n] as
// [B, T, d_mlp, d_model] per layer, stack_neuron_results(apply_ln=True) concatenates the layers into [L * d_mlp, B, T, d_model]
// ("SUPER expensive"), subtracts each row's mean and divides by the cached fp32 hook_scale of the LayerNorm the neurons feed; the
// user multiplies with the answer directions.  A neuron's result is ONE row of W_out times a number, so with
// (r - mean(r) 1) . a = r . (a - mean(a) 1) the whole composition is elementwise (M = d_mlp):
//
//   attr[b, t, l M + n, o] = post_l[b, t, n] G[l, g(b) + o, n] / scale[b, t],     G[l, r, n] = sum_k W_out_l[n, k] (a[r, k] - mean(a[r, :]))
//
// G is what attr_fold_kernel (attribution.hip) computes for any row-major bf16 [HD, d_model] matrix: W_out folds with HD = d_mlp.
//
// The value, the same bits in both kernels (nattr_value):  v = fdiv_rn(fmul_rn(post, G), scale), post the bf16 tap element widened
// to fp32; a product that is not finite is stored as the canonical NaN 0x7fc00000, so a neuron whose post is NaN or +-inf is NaN in
// every answer column (the reference's mean over that neuron's d_model values is not finite) and its neighbours never see it;
// post == 0 gives exactly +-0.
//
//   nattr_dense_kernel<OC>   out[ro, l M + n, o], fp32 [B, T_out, L M, O].  A lane owns 8 consecutive neurons (16 bytes of the tap) and
//                            keeps its 8 x OC values of G (OC = 1 / 4 / 16 >= O) in registers for all rows of its tile, so a tap
//                            element is loaded once for up to 16 answers; the next pass's 16 bytes are fetched before the current
//                            pass's arithmetic.  Rows are tiled per SEGMENT as in attr_head_kernel (shared answers: one segment;
//                            per image: B segments, G rows at seg * O); `pos` maps output row ro to tap row ro * T + pos.  No LDS.
//   nattr_topk_kernel        per (output row, answer) the k entries of the L M values with the largest key, key = v (by = 0) or |v|
//                            (by = 1) compared as floats: -0 equals +0, NaN above everything (torch.topk's order), ties to the lowest
//                            flat index l M + n, the output sorted by that order.  One workgroup per (row, answer), the algorithm of
//                            sae_topk_row_lds (sae.hpp) on values computed on the fly: per-thread maximum -> the k-th of the 256
//                            maxima as threshold (at least k values reach it) -> a second pass over the chunks of those threads
//                            alone whose own maximum reaches the threshold, shared out over the workgroup, compacts the
//                            candidates into LDS -> exact rank by (key, index).  With 0 < scale < inf the first pass takes the
//                            maximum over the PRODUCTS (fl(x / scale) is monotone) and divides once per thread.  More
//                            than NATTR_CAP candidates (a mass tie at the top: rows of zeros): an MSB-first radix select of the
//                            k-th key, then the keys above it ranked in LDS and the ties taken in index order.  val carries the
//                            bits the dense kernel stores at idx.  The second pass and the other answers' workgroups of the same
//                            row (consecutive block ids) find the row in the L2: L M 2 bytes, 73 KB at B/32.
//
// Error of a finite dense element against the exact value (u = 2^-24, d = d_model): the fold leaves (d + 2) u + (d + 1) u on
// sum_k |W_nk| (|a_k| + mean|a|) (attribution.hip), the product and the division one rounding each:
//   |got - exact| <= (2 d + 8) u |post| sum_k |W_nk| (|a_k| + mean_k |a_k|) / scale                 (tests/_neuron_attribution_cases.py)
#include "attribution.hpp"

namespace {

constexpr int NATTR_CAP = 1024;              // candidate capacity of the top-k's streaming pass (more: the radix-select passes)

__device__ __forceinline__ float nattr_finish(float prod, float scale) {
    return (fabsf(prod) <= 3.402823466e38f) ? __fdiv_rn(prod, scale) : __uint_as_float(0x7fc00000u);
}
__device__ __forceinline__ float nattr_value(float post, float g, float scale) { return nattr_finish(__fmul_rn(post, g), scale); }

// the order-preserving uint image of the key: NaN on top, -0 folded onto +0
__device__ __forceinline__ uint32_t nattr_key(float v, int by) {
    uint32_t u = __float_as_uint(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    if (by) u &= 0x7fffffffu;
    if ((u & 0x7fffffffu) == 0u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct NAttrDenseParams {
    AttrPtrs post;              // the L taps, [N][M] bf16 each
    const float* G;             // [L][R][M]
    const float* scale;         // [N]
    float* out;                 // [rows_out][L * M][O]
    int32_t M, MC, L, O, R;     // MC = M / 8: 16-byte chunks of a tap row
    int32_t T, pos;             // pos < 0: every token
    int32_t seg_rows;           // output rows per segment
    int32_t n_seg;              // 1 (shared answers) or B (per image: G rows start at seg * O)
    int32_t per_image;
    int32_t CG, n_cg;           // chunks per workgroup (<= 256), chunk groups
    int32_t RP, passes;         // rows per pass = 256 / CG; a tile is RP * passes rows
    int32_t n_tile;             // row tiles per segment
};

// grid.x = L * n_seg * n_tile * n_cg (chunk group fastest); 256 threads
template <int OC>
__global__ __launch_bounds__(256) void nattr_dense_kernel(const NAttrDenseParams p) {
    static_assert(OC == 1 || OC == 4 || OC == 16, "answers held in registers");
    int w = blockIdx.x;
    const int cg = w % p.n_cg; w /= p.n_cg;
    const int tile = w % p.n_tile; w /= p.n_tile;
    const int seg = w % p.n_seg;
    const int l = w / p.n_seg;

    const int tid = threadIdx.x;
    const int rip = tid / p.CG, c = cg * p.CG + (tid - rip * p.CG);
    const bool active = (rip < p.RP) & (c < p.MC);

    // this lane's 8 x OC values of G, kept for every row of the tile
    float g[OC][8];
#pragma unroll
    for (int o = 0; o < OC; ++o) {
#pragma unroll
        for (int i = 0; i < 8; ++i) g[o][i] = 0.0f;
        if (active && o < p.O) {
            const int64_t row = (int64_t)l * p.R + (p.per_image ? seg * p.O : 0) + o;
            load8(p.G + row * p.M + c * 8, g[o]);
        }
    }

    const bf16_t* post = reinterpret_cast<const bf16_t*>(p.post.ptr[l]);
    const int64_t C = (int64_t)p.L * p.M;
    const int row_begin = tile * p.RP * p.passes;
    // the 16 bytes of this lane in pass ps (zeros outside the segment): fetched one pass ahead of their use
    auto fetch = [&](int ps) -> uint4 {
        const int lrow = row_begin + ps * p.RP + rip;
        if (!(active & (ps < p.passes) & (lrow < p.seg_rows))) return make_uint4(0u, 0u, 0u, 0u);
        const int64_t ro = (int64_t)seg * p.seg_rows + lrow;
        const int64_t n = p.pos < 0 ? ro : ro * p.T + p.pos;
        return *reinterpret_cast<const uint4*>(post + n * p.M + c * 8);
    };
    uint4 next = fetch(0);
    for (int ps = 0; ps < p.passes; ++ps) {
        const int lrow = row_begin + ps * p.RP + rip;                        // row inside the segment
        const bool valid = active & (lrow < p.seg_rows);
        const int64_t ro = (int64_t)seg * p.seg_rows + lrow;                // output row
        const int64_t n = p.pos < 0 ? ro : ro * p.T + p.pos;                // tap row
        const uint4 q = next;
        next = fetch(ps + 1);
        if (!valid) continue;
        const float v[8] = {__uint_as_float(q.x << 16), __uint_as_float(q.x & 0xffff0000u), __uint_as_float(q.y << 16),
                            __uint_as_float(q.y & 0xffff0000u), __uint_as_float(q.z << 16), __uint_as_float(q.z & 0xffff0000u),
                            __uint_as_float(q.w << 16), __uint_as_float(q.w & 0xffff0000u)};
        const float scale = p.scale[n];
        float* out = p.out + (ro * C + (int64_t)l * p.M + c * 8) * p.O;     // this lane's 8 x O consecutive floats
        if (p.O == OC) {
            // the lane's floats are whole 16-byte words (out is 16-byte aligned, the offset a multiple of 8 O floats)
            if constexpr (OC == 1) {
                float r[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) r[i] = nattr_value(v[i], g[0][i], scale);
                store8(out, r);
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
#pragma unroll
                    for (int o = 0; o < OC; o += 4)
                        *reinterpret_cast<float4*>(out + i * OC + o) =
                            make_float4(nattr_value(v[i], g[o][i], scale), nattr_value(v[i], g[o + 1][i], scale),
                                        nattr_value(v[i], g[o + 2][i], scale), nattr_value(v[i], g[o + 3][i], scale));
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
#pragma unroll
                for (int o = 0; o < OC; ++o)
                    if (o < p.O) out[i * p.O + o] = nattr_value(v[i], g[o][i], scale);
            }
        }
    }
}

struct NAttrTopkParams {
    AttrPtrs post;              // the L taps, [N][M] bf16 each
    const float* G;             // [L][R][M]
    const float* scale;         // [N]
    float* val;                 // [rows_out][O][k]
    int32_t* idx;               // [rows_out][O][k]: flat index l * M + n
    int32_t M, MC, L, O, R;
    int32_t T, T_out, pos;
    int32_t per_image, k, by;
};

// grid.x = rows_out * O (answer fastest: the workgroups of one tap row are neighbours); 256 threads
__global__ __launch_bounds__(256) void nattr_topk_kernel(const NAttrTopkParams p) {
    __shared__ const bf16_t* tap[PV_ATTR_MAX_LAYERS];
    __shared__ __attribute__((aligned(16))) uint32_t hist[256];
    __shared__ uint32_t cand_key[NATTR_CAP];
    __shared__ int32_t cand_idx[NATTR_CAP];
    __shared__ uint16_t qlist[256];
    __shared__ uint32_t sh_T0, sh_ncand, sh_nq, sh_prefix, sh_k, sh_wcnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t ro = blockIdx.x / (unsigned)p.O;
    const int o = (int)(blockIdx.x - ro * p.O);
    const int64_t nrow = p.pos < 0 ? ro : ro * p.T + p.pos;                  // tap row
    const int64_t grow = (p.per_image ? (ro / p.T_out) * p.O : 0) + o;       // row of G inside a layer
    const int k = p.k, by = p.by, M = p.M, MC = p.MC;
    const int nchunks = p.L * MC;

    // the tap pointers by constant index (a lane-dependent index into the kernel arguments would put them in scratch)
#pragma unroll
    for (int l = 0; l < PV_ATTR_MAX_LAYERS; ++l)
        if (tid == l) tap[l] = reinterpret_cast<const bf16_t*>(p.post.ptr[l]);
    if (tid == 0) { sh_T0 = 0u; sh_ncand = 0u; sh_nq = 0u; }
    __syncthreads();
    const float scale = p.scale[nrow];
    const float* Grow = p.G + grow * M;
    const int64_t Gstride = (int64_t)p.R * M;

    // the products post G of chunk q = l * MC + c: the 8 neurons c * 8 .. of layer l, flat indices q * 8 ..
    auto chunk_prods = [&](int l, int c, float (&prod)[8]) {
        float pv[8], gv[8];
        load8(tap[l] + nrow * M + c * 8, pv);
        load8(Grow + l * Gstride + c * 8, gv);
#pragma unroll
        for (int i = 0; i < 8; ++i) prod[i] = __fmul_rn(pv[i], gv[i]);
    };
    auto chunk_keys = [&](int q, uint32_t (&key)[8]) {
        float prod[8];
        chunk_prods(q / MC, q % MC, prod);
#pragma unroll
        for (int i = 0; i < 8; ++i) key[i] = nattr_key(nattr_finish(prod[i], scale), by);
    };
    auto value_at = [&](int flat) -> float {
        const int l = flat / M, n = flat - l * M;
        return nattr_value(bf16_to_f32(tap[l][nrow * M + n]), Grow[l * Gstride + n], scale);
    };
    int32_t* idx_out = p.idx + (int64_t)blockIdx.x * k;
    float* val_out = p.val + (int64_t)blockIdx.x * k;

    uint32_t lmax = 0;                                                       // (no key is 0: threads without a chunk stay below every value)
    if (scale > 0.0f && scale <= 3.402823466e38f) {
        // the usual row: fl(prod / scale) does not decrease with prod, nor its magnitude with |prod|, so the thread's largest key is
        // the key of its largest product (or NaN, if any product is not finite) -- one division per thread, not one per element
        float fmx = -3.402823466e38f;
        uint32_t amx = 0;
        int l = tid / MC, c = tid - l * MC;
        const int step_l = 256 / MC, step_c = 256 - step_l * MC;
        // four chunks per round, their 48 bytes each requested before the first is used (past the row's end: nothing is loaded or counted)
        for (int q = tid; q < nchunks; q += 4 * 256) {
            uint4 pv[4];
            float4 ga[4], gb[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                pv[u] = make_uint4(0u, 0u, 0u, 0u);
                ga[u] = gb[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (q + 256 * u < nchunks) {
                    const float* g = Grow + l * Gstride + c * 8;
                    pv[u] = *reinterpret_cast<const uint4*>(tap[l] + nrow * M + c * 8);
                    ga[u] = *reinterpret_cast<const float4*>(g);
                    gb[u] = *reinterpret_cast<const float4*>(g + 4);
                }
                l += step_l; c += step_c;
                if (c >= MC) { c -= MC; ++l; }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (q + 256 * u >= nchunks) continue;
                const float prod[8] = {__fmul_rn(__uint_as_float(pv[u].x << 16), ga[u].x), __fmul_rn(__uint_as_float(pv[u].x & 0xffff0000u), ga[u].y),
                                       __fmul_rn(__uint_as_float(pv[u].y << 16), ga[u].z), __fmul_rn(__uint_as_float(pv[u].y & 0xffff0000u), ga[u].w),
                                       __fmul_rn(__uint_as_float(pv[u].z << 16), gb[u].x), __fmul_rn(__uint_as_float(pv[u].z & 0xffff0000u), gb[u].y),
                                       __fmul_rn(__uint_as_float(pv[u].w << 16), gb[u].z), __fmul_rn(__uint_as_float(pv[u].w & 0xffff0000u), gb[u].w)};
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    amx = max(amx, __float_as_uint(prod[i]) & 0x7fffffffu);
                    fmx = fmaxf(fmx, prod[i]);
                }
            }
        }
        if (tid < nchunks) lmax = amx >= 0x7f800000u ? 0xffffffffu : nattr_key(nattr_finish(by ? __uint_as_float(amx) : fmx, scale), by);
    } else {
        for (int q = tid; q < nchunks; q += 256) {
            uint32_t key[8];
            chunk_keys(q, key);
#pragma unroll
            for (int i = 0; i < 8; ++i) lmax = max(lmax, key[i]);
        }
    }
    hist[tid] = lmax;
    __syncthreads();
    {
        uint32_t rank = 0;
        for (int u = 0; u < 256; u += 4) {
            const uint4 x = *reinterpret_cast<const uint4*>(&hist[u]);       // same address for all lanes: LDS broadcast
            rank += (x.x > lmax) || (x.x == lmax && u < tid);
            rank += (x.y > lmax) || (x.y == lmax && u + 1 < tid);
            rank += (x.z > lmax) || (x.z == lmax && u + 2 < tid);
            rank += (x.w > lmax) || (x.w == lmax && u + 3 < tid);
        }
        if (rank == (uint32_t)(k - 1)) sh_T0 = lmax;                         // k <= 256: exactly one thread
    }
    __syncthreads();
    const uint32_t T0 = sh_T0;
    // only the chunks of a thread whose own maximum reaches T0 hold candidates: those threads are listed, and their chunks (q = thread
    // + 256 it) are shared out over the whole workgroup
    if (lmax >= T0 && tid < nchunks) qlist[atomicAdd(&sh_nq, 1u)] = (uint16_t)tid;
    __syncthreads();
    const int iters = (nchunks + 255) / 256, n_work = (int)sh_nq * iters;
    for (int w = tid; w < n_work; w += 256) {
        const int j = w / iters, q = qlist[j] + 256 * (w - j * iters);
        if (q >= nchunks) continue;
        uint32_t key[8];
        chunk_keys(q, key);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (key[i] >= T0) {
                const uint32_t at = atomicAdd(&sh_ncand, 1u);
                if (at < NATTR_CAP) { cand_key[at] = key[i]; cand_idx[at] = q * 8 + i; }
            }
        }
    }
    __syncthreads();
    const uint32_t ncand = sh_ncand;
    if (ncand <= NATTR_CAP) {
        for (uint32_t c = tid; c < ncand; c += 256) {
            const uint32_t kc = cand_key[c];
            const int32_t ic = cand_idx[c];
            uint32_t rank = 0;
            for (uint32_t x = 0; x < ncand; ++x) {
                const uint32_t kx = cand_key[x];
                rank += (kx > kc) || (kx == kc && cand_idx[x] < ic);
            }
            if (rank < (uint32_t)k) {
                idx_out[rank] = ic;
                val_out[rank] = value_at(ic);
            }
        }
        return;
    }

    // ---------------------------------------------------- fallback: radix select of the k-th key, re-streaming the row
    uint32_t prefix = 0, kk = (uint32_t)k;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        __syncthreads();
        hist[tid] = 0;
        __syncthreads();
        const uint32_t hi_mask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
        for (int q = tid; q < nchunks; q += 256) {
            uint32_t key[8];
            chunk_keys(q, key);
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if ((key[i] & hi_mask) == (prefix & hi_mask)) atomicAdd(&hist[(key[i] >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t acc = 0;
            int dsel = 0;
            for (int dgt = 255; dgt >= 0; --dgt) {
                if (acc + hist[dgt] >= kk) { dsel = dgt; break; }
                acc += hist[dgt];
            }
            sh_prefix = prefix | ((uint32_t)dsel << shift);
            sh_k = kk - acc;
        }
        __syncthreads();
        prefix = sh_prefix;
        kk = sh_k;
    }
    // prefix = the k-th largest key; k - kk < k keys lie above it.  Every thread now walks a CONTIGUOUS range of chunks, so that a
    // scan over the threads counts the ties in index order: the first kk of them follow the keys above.
    const uint32_t n_gt = (uint32_t)k - kk;
    const int cpt = (nchunks + 255) / 256;
    const int q_begin = min(tid * cpt, nchunks), q_end = min(q_begin + cpt, nchunks);
    uint32_t neq = 0;
    for (int q = q_begin; q < q_end; ++q) {
        uint32_t key[8];
        chunk_keys(q, key);
#pragma unroll
        for (int i = 0; i < 8; ++i) neq += key[i] == prefix;
    }
    uint32_t pos_eq;
    {
        uint32_t inc = neq;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const uint32_t a = __shfl_up(inc, s, 64);
            if (lane >= s) inc += a;
        }
        if (lane == 63) sh_wcnt[wave] = inc;
        if (tid == 0) sh_ncand = 0u;
        __syncthreads();
        uint32_t base = 0;
        for (int x = 0; x < 4; ++x)
            if (x < wave) base += sh_wcnt[x];
        pos_eq = base + inc - neq;
    }
    for (int q = q_begin; q < q_end; ++q) {
        uint32_t key[8];
        chunk_keys(q, key);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (key[i] > prefix) {
                const uint32_t at = atomicAdd(&sh_ncand, 1u);                // n_gt < k <= 256 <= NATTR_CAP of them
                if (at < NATTR_CAP) { cand_key[at] = key[i]; cand_idx[at] = q * 8 + i; }
            } else if (key[i] == prefix) {
                if (pos_eq < kk) {
                    idx_out[n_gt + pos_eq] = q * 8 + i;
                    val_out[n_gt + pos_eq] = value_at(q * 8 + i);
                }
                ++pos_eq;
            }
        }
    }
    __syncthreads();
    const uint32_t ngt = min(sh_ncand, (uint32_t)NATTR_CAP);
    for (uint32_t c = tid; c < ngt; c += 256) {
        const uint32_t kc = cand_key[c];
        const int32_t ic = cand_idx[c];
        uint32_t rank = 0;
        for (uint32_t x = 0; x < ngt; ++x) {
            const uint32_t kx = cand_key[x];
            rank += (kx > kc) || (kx == kc && cand_idx[x] < ic);
        }
        if (rank < n_gt) {
            idx_out[rank] = ic;
            val_out[rank] = value_at(ic);
        }
    }
}

// the checks both entry points share; R = answer rows of the fold
int nattr_check(const char* who, int32_t dtype, const void* const* post, const void* const* W_out, int32_t n_layers, int32_t n_images,
                int32_t n_tokens, int32_t pos, int32_t d_mlp, int32_t d_model, const float* scale, const float* answers,
                int32_t n_answers, int32_t per_image, const void* workspace, size_t workspace_bytes, int64_t* R_out) {
    const std::string w(who);
    PV_REQUIRE(dtype == PV_DTYPE_BF16, w + ": the taps and W_out must be bf16 (dtype PV_DTYPE_BF16); fp32 is not served");
    PV_REQUIRE(d_mlp >= 8 && d_mlp % 8 == 0, w + ": d_mlp must be a multiple of 8 (a lane owns 16 bytes of a tap row)");
    PV_REQUIRE(d_model >= 8 && d_model % 8 == 0, w + ": d_model must be a multiple of 8 (16-byte operand chunks)");
    PV_REQUIRE(n_layers >= 1 && n_layers <= PV_ATTR_MAX_LAYERS,
               w + ": n_layers must be between 1 and PV_ATTR_MAX_LAYERS = " PV_STR(PV_ATTR_MAX_LAYERS));
    PV_REQUIRE(n_answers >= 1 && n_answers <= PV_ATTR_MAX_ANSWERS,
               w + ": n_answers must be between 1 and PV_ATTR_MAX_ANSWERS = " PV_STR(PV_ATTR_MAX_ANSWERS));
    PV_REQUIRE(n_images >= 1 && n_tokens >= 1, w + ": n_images and n_tokens must be positive");
    PV_REQUIRE(pos >= -1 && pos < n_tokens, w + ": pos must be -1 (every token) or a token index below n_tokens");
    PV_REQUIRE(post && W_out && scale && answers && workspace, w + ": post, W_out, scale, answers and workspace must not be NULL");
    PV_REQUIRE(pv_aligned16(answers) && pv_aligned16(workspace) && (reinterpret_cast<uintptr_t>(scale) & 3u) == 0,
               w + ": answers and workspace must be 16-byte aligned, scale 4-byte aligned");
    for (int l = 0; l < n_layers; ++l)
        PV_REQUIRE(post[l] && W_out[l] && pv_aligned16(post[l]) && pv_aligned16(W_out[l]),
                   w + ": every tap and every W_out must be a 16-byte aligned device pointer");
    PV_REQUIRE((uint64_t)n_images * (uint64_t)n_tokens * (uint64_t)d_mlp * 2 < (1ull << 32), w + ": a tap must stay below 4 GiB");
    const int64_t R = per_image ? (int64_t)n_images * n_answers : n_answers;
    PV_REQUIRE(d_mlp < (1 << 24) && R < (1 << 30), w + ": d_mlp or the number of answer rows is out of range");
    if (workspace_bytes < pv_neuron_attribution_workspace_bytes(n_layers, d_mlp, (int32_t)R)) {
        pv_set_error(w + ": workspace too small (pv_neuron_attribution_workspace_bytes)");
        return PV_ERR_WORKSPACE;
    }
    *R_out = R;
    return PV_OK;
}

}  // namespace

extern "C" size_t pv_neuron_attribution_workspace_bytes(int32_t n_layers, int32_t d_mlp, int32_t n_answer_rows) {
    if (n_layers <= 0 || d_mlp <= 0 || n_answer_rows <= 0) return 0;
    return (size_t)pv_align_up((int64_t)n_layers * n_answer_rows * d_mlp * 4, 256);
}

extern "C" int pv_neuron_attribution(int32_t dtype, const void* const* post, const void* const* W_out, int32_t n_layers, int32_t n_images,
                                     int32_t n_tokens, int32_t pos, int32_t d_mlp, int32_t d_model, const float* scale,
                                     const float* answers, int32_t n_answers, int32_t per_image, float* out, void* workspace,
                                     size_t workspace_bytes, void* stream_) {
    const char* who = "neuron attribution";
    PV_REQUIRE(out && pv_aligned16(out), "neuron attribution: out must be a 16-byte aligned device pointer");
    int64_t R = 0;
    if (const int rc = nattr_check(who, dtype, post, W_out, n_layers, n_images, n_tokens, pos, d_mlp, d_model, scale, answers, n_answers,
                                   per_image, workspace, workspace_bytes, &R))
        return rc;
    NAttrDenseParams p{};
    for (int l = 0; l < n_layers; ++l) p.post.ptr[l] = post[l];
    float* G = reinterpret_cast<float*>(workspace);
    p.G = G; p.scale = scale; p.out = out;
    p.M = d_mlp; p.MC = d_mlp / 8; p.L = n_layers; p.O = n_answers; p.R = (int32_t)R;
    p.T = n_tokens; p.pos = pos;
    const int t_out = pos < 0 ? n_tokens : 1;
    p.per_image = per_image ? 1 : 0;
    p.n_seg = per_image ? n_images : 1;
    p.seg_rows = per_image ? t_out : n_images * t_out;
    p.n_cg = (p.MC + 255) / 256;
    p.CG = (p.MC + p.n_cg - 1) / p.n_cg;                     // the chunks spread evenly over the groups (3072: two groups of 192)
    p.RP = 256 / p.CG;
    p.passes = (32 + p.RP - 1) / p.RP;                       // tiles of about 32 rows: G is fetched once per tile
    const int tile_rows = p.RP * p.passes;
    p.n_tile = (p.seg_rows + tile_rows - 1) / tile_rows;
    const int64_t blocks = (int64_t)n_layers * p.n_seg * p.n_tile * p.n_cg;
    PV_REQUIRE(blocks < (1ll << 31), "neuron attribution: the launch would need 2^31 workgroups or more");

    if (const int rc = attr_launch_fold(who, W_out, n_layers, d_mlp, d_model, R, answers, G, reinterpret_cast<hipStream_t>(stream_)))
        return rc;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const dim3 grid((unsigned)blocks);
    if (p.O == 1) hipLaunchKernelGGL(nattr_dense_kernel<1>, grid, dim3(256), 0, stream, p);
    else if (p.O <= 4) hipLaunchKernelGGL(nattr_dense_kernel<4>, grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(nattr_dense_kernel<16>, grid, dim3(256), 0, stream, p);
    PV_LAUNCH_CHECK("nattr_dense_kernel");
    return PV_OK;
}

extern "C" int pv_neuron_attribution_topk(int32_t dtype, const void* const* post, const void* const* W_out, int32_t n_layers,
                                          int32_t n_images, int32_t n_tokens, int32_t pos, int32_t d_mlp, int32_t d_model,
                                          const float* scale, const float* answers, int32_t n_answers, int32_t per_image, int32_t k,
                                          int32_t by, float* val, int32_t* idx, void* workspace, size_t workspace_bytes, void* stream_) {
    const char* who = "neuron attribution top-k";
    PV_REQUIRE(val && idx && (reinterpret_cast<uintptr_t>(val) & 3u) == 0 && (reinterpret_cast<uintptr_t>(idx) & 3u) == 0,
               "neuron attribution top-k: val and idx must be 4-byte aligned device pointers");
    PV_REQUIRE(by == 0 || by == 1, "neuron attribution top-k: by must be 0 (the value) or 1 (its magnitude)");
    PV_REQUIRE(k >= 1 && k <= PV_NATTR_MAX_K, "neuron attribution top-k: k must be between 1 and PV_NATTR_MAX_K = " PV_STR(PV_NATTR_MAX_K));
    int64_t R = 0;
    if (const int rc = nattr_check(who, dtype, post, W_out, n_layers, n_images, n_tokens, pos, d_mlp, d_model, scale, answers, n_answers,
                                   per_image, workspace, workspace_bytes, &R))
        return rc;
    PV_REQUIRE((int64_t)k <= (int64_t)n_layers * d_mlp, "neuron attribution top-k: k must not exceed n_layers * d_mlp");
    NAttrTopkParams p{};
    for (int l = 0; l < n_layers; ++l) p.post.ptr[l] = post[l];
    float* G = reinterpret_cast<float*>(workspace);
    p.G = G; p.scale = scale; p.val = val; p.idx = idx;
    p.M = d_mlp; p.MC = d_mlp / 8; p.L = n_layers; p.O = n_answers; p.R = (int32_t)R;
    p.T = n_tokens; p.T_out = pos < 0 ? n_tokens : 1; p.pos = pos;
    p.per_image = per_image ? 1 : 0; p.k = k; p.by = by;
    const int64_t blocks = (int64_t)n_images * p.T_out * n_answers;
    PV_REQUIRE(blocks < (1ll << 31), "neuron attribution top-k: the launch would need 2^31 workgroups or more");

    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (const int rc = attr_launch_fold(who, W_out, n_layers, d_mlp, d_model, R, answers, G, stream)) return rc;
    hipLaunchKernelGGL(nattr_topk_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, p);
    PV_LAUNCH_CHECK("nattr_topk_kernel");
    return PV_OK;
}
