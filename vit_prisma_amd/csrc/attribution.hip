// Direct logit attribution by attention head on the cached hook_z taps (gfx950).
//
// Reference semantics (activation_cache.py:388-490, :656-735): compute_head_results materialises r = z[..., h, :] @ W_O[h] as
// [B, T, H, d_model] per layer, stack_head_results(apply_ln=True) concatenates the layers into [L * H, B, T, d_model], subtracts
// each row's mean and divides by the cached fp32 hook_scale of the LayerNorm the heads feed; the user multiplies with the answer
// directions.  None of the [..., d_model] tensors is needed.  For one head result r = z_h @ W_O[h] and an answer a:
//
//   ((r - mean(r) 1) . a) / scale  =  (sum_e z[h, e] G[h, e]) / scale,      G[h, e] = sum_k W_O[h, e, k] (a_k - mean(a))
//
// because (r - mean(r) 1) . a = r . (a - mean(a) 1).  G is [L, H * d_head] per answer row; what remains is one pass over the taps.
//
//   attr_fold_kernel          G[l, r, j] = sum_k W_O_l[j, k] ac[r, k],  ac[r, :] = a[r, :] - mean(a[r, :]), everything fp32 (VALU):
//                             a workgroup per (layer, 64 columns j, 16 answer rows r), W_O and ac staged through LDS in K slabs of 64
//   attr_head_kernel<LPH, OC> out[n, l * H + h, o] = (sum_e z_l[n, h, e] G[l, g(n) + o, h * d_head + e]) / scale[n]
//                             LPH lanes share a head (8 bf16 = 16 bytes of z each: 4 lanes at d_head 32, 8 at 64, 16 for the wide
//                             heads, whose lanes past d_head / 8 hold zeros); a lane keeps ITS head's 8 x OC values of G in registers
//                             for all rows of the workgroup's tile, so a tap element is loaded once for up to OC = 16 answers.
// Row mapping of the head kernel: the output has rows_out = B * T_out rows (T_out = T, or 1 with a `pos`), row ro reads tap row
// ro (pos < 0) or ro * T + pos.  Row tiles are counted per SEGMENT: one segment of B * T_out rows when the answers are shared, B
// segments of T_out rows when each image has its own -- a workgroup then never holds rows of two images and its G rows start at
// seg * O.
//
// Non-finite heads: a head whose z holds a NaN or an infinity has a non-finite mean in the reference and is NaN in every answer
// column; here a dot product that is not finite is stored as NaN (inf * G alone would leave +-inf).  Other heads of the row do
// not see that head's z and stay finite.
//
// Error of a finite element against the exact value (u = 2^-24, d = d_model): the fp32 mean of a (d terms, one division) and the
// subtraction leave |ac^_k - ac_k| <= (d + 2) u (|a_k| + mean_k |a_k|); the d products and the sum of d terms for G add
// (d + 1) u, the d_head products and their sum (d_head + 1) u, the division u:
//   |got - exact| <= (2 d + d_head + 8) u sum_e |z_e| sum_k |W_ek| (|a_k| + mean_k |a_k|) / scale       (tests/_attribution_cases.py)
// (products enter the sums by fmaf, one rounding per term, so the form is inside what the bound allows for mul + add.)
#include "attribution.hpp"

namespace {

// grid = (ceil(HD / 64), ceil(R / 16), L); 256 threads: thread (jj = tid & 63, rg = tid >> 6) owns column j0 + jj of rows r0 + 4 rg .. + 3
__global__ __launch_bounds__(256) void attr_fold_kernel(const AttrPtrs W_O, const float* __restrict__ answers, int HD, int d, int R,
                                                        float* __restrict__ G) {
    __shared__ __attribute__((aligned(16))) float Ws[FOLD_TJ][FOLD_WS];
    __shared__ __attribute__((aligned(16))) float As[FOLD_TR][FOLD_KC];
    __shared__ float smean[FOLD_TR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j0 = blockIdx.x * FOLD_TJ, r0 = blockIdx.y * FOLD_TR, l = blockIdx.z;
    const bf16_t* W = reinterpret_cast<const bf16_t*>(W_O.ptr[l]);

    // the means of this tile's answer rows: wave w takes rows 4 w .. 4 w + 3 (the same order in every workgroup)
    for (int i = 0; i < 4; ++i) {
        const int row = wave * 4 + i;
        float sum = 0.0f;
        if (r0 + row < R) {
            const float* a = answers + (int64_t)(r0 + row) * d;
            for (int k = 4 * lane; k < d; k += 256) {
                const float4 v = *reinterpret_cast<const float4*>(a + k);
                sum += (v.x + v.y) + (v.z + v.w);
            }
        }
        sum = wave_sum(sum);
        if (lane == 0) smean[row] = sum / (float)d;
    }
    __syncthreads();

    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int k0 = 0; k0 < d; k0 += FOLD_KC) {
        // W_O slab: 64 rows x 64 k bf16, two 16-byte chunks per thread; outside [HD) x [d): zeros
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int idx = p * 256 + tid, row = idx >> 3, kc = (idx & 7) * 8;
            float v[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            if (j0 + row < HD && k0 + kc < d) load8(W + (int64_t)(j0 + row) * d + k0 + kc, v);
            *reinterpret_cast<float4*>(&Ws[row][kc]) = make_float4(v[0], v[1], v[2], v[3]);
            *reinterpret_cast<float4*>(&Ws[row][kc + 4]) = make_float4(v[4], v[5], v[6], v[7]);
        }
        // centred answers: 16 rows x 64 k fp32, one 16-byte chunk per thread; outside [R) x [d): zeros (not -mean)
        {
            const int row = tid >> 4, kc = (tid & 15) * 4;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (r0 + row < R && k0 + kc < d) {
                v = *reinterpret_cast<const float4*>(answers + (int64_t)(r0 + row) * d + k0 + kc);
                const float m = smean[row];
                v.x -= m; v.y -= m; v.z -= m; v.w -= m;
            }
            *reinterpret_cast<float4*>(&As[row][kc]) = v;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < FOLD_KC; k += 4) {
            const float4 w = *reinterpret_cast<const float4*>(&Ws[lane][k]);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float4 a = *reinterpret_cast<const float4*>(&As[wave * 4 + i][k]);
                acc[i] = fmaf(w.x, a.x, acc[i]);
                acc[i] = fmaf(w.y, a.y, acc[i]);
                acc[i] = fmaf(w.z, a.z, acc[i]);
                acc[i] = fmaf(w.w, a.w, acc[i]);
            }
        }
        __syncthreads();
    }
    const int j = j0 + lane;
    if (j < HD) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = r0 + wave * 4 + i;
            if (r < R) G[((int64_t)l * R + r) * HD + j] = acc[i];
        }
    }
}

struct AttrHeadParams {
    AttrPtrs z;                 // the L taps, [N][H][d_head] bf16 each
    const float* G;             // [L][R][HD]
    const float* scale;         // [N]
    float* out;                 // [rows_out][L * H][O]
    int32_t H, dh, L, O, R;
    int32_t T, pos;             // pos < 0: every token
    int32_t seg_rows;           // output rows per segment
    int32_t n_seg;              // 1 (shared answers) or B (per image: G rows start at seg * O)
    int32_t per_image;
    int32_t HG;                 // heads per workgroup: min(H, 256 / LPH)
    int32_t RP, passes;         // rows per pass = 256 / (HG * LPH); a tile is RP * passes rows
    int32_t n_tile, n_hg;       // row tiles per segment, head groups
};

// grid.x = L * n_seg * n_tile * n_hg (head group fastest); 256 threads
template <int LPH, int OC>
__global__ __launch_bounds__(256) void attr_head_kernel(const AttrHeadParams p) {
    static_assert(LPH == 4 || LPH == 8 || LPH == 16, "lanes per head");
    static_assert(OC == 1 || OC == 4 || OC == 16, "answers held in registers");
    int w = blockIdx.x;
    const int hg = w % p.n_hg; w /= p.n_hg;
    const int tile = w % p.n_tile; w /= p.n_tile;
    const int seg = w % p.n_seg;
    const int l = w / p.n_seg;

    const int tid = threadIdx.x;
    const int c = tid & (LPH - 1), slot = tid / LPH;
    const int rip = slot / p.HG, h = hg * p.HG + (slot - rip * p.HG);
    const bool active = (rip < p.RP) & (h < p.H) & (c * 8 < p.dh);
    const int HD = p.H * p.dh;

    // this lane's 8 x OC values of G, kept for every row of the tile
    float g[OC][8];
#pragma unroll
    for (int o = 0; o < OC; ++o) {
#pragma unroll
        for (int i = 0; i < 8; ++i) g[o][i] = 0.0f;
        if (active && o < p.O) {
            const int64_t row = (int64_t)l * p.R + (p.per_image ? seg * p.O : 0) + o;
            load8(p.G + row * HD + h * p.dh + c * 8, g[o]);
        }
    }

    const bf16_t* z = reinterpret_cast<const bf16_t*>(p.z.ptr[l]);
    const int C = p.L * p.H;
    const int row_begin = tile * p.RP * p.passes;
    // the 16 bytes of this lane in pass ps (zeros outside the segment): fetched one pass ahead of their use
    auto fetch = [&](int ps) -> uint4 {
        const int lrow = row_begin + ps * p.RP + rip;
        if (!(active & (ps < p.passes) & (lrow < p.seg_rows))) return make_uint4(0u, 0u, 0u, 0u);
        const int64_t ro = (int64_t)seg * p.seg_rows + lrow;
        const int64_t n = p.pos < 0 ? ro : ro * p.T + p.pos;
        return *reinterpret_cast<const uint4*>(z + (n * p.H + h) * p.dh + c * 8);
    };
    uint4 next = fetch(0);
    for (int ps = 0; ps < p.passes; ++ps) {
        const int lrow = row_begin + ps * p.RP + rip;                        // row inside the segment
        const bool valid = active & (lrow < p.seg_rows);
        const int64_t ro = (int64_t)seg * p.seg_rows + lrow;                // output row
        const int64_t n = p.pos < 0 ? ro : ro * p.T + p.pos;                // tap row
        const uint4 q = next;
        next = fetch(ps + 1);
        const float v[8] = {__uint_as_float(q.x << 16), __uint_as_float(q.x & 0xffff0000u), __uint_as_float(q.y << 16),
                            __uint_as_float(q.y & 0xffff0000u), __uint_as_float(q.z << 16), __uint_as_float(q.z & 0xffff0000u),
                            __uint_as_float(q.w << 16), __uint_as_float(q.w & 0xffff0000u)};
        float acc[OC];
#pragma unroll
        for (int o = 0; o < OC; ++o) {
            float s = 0.0f;
#pragma unroll
            for (int i = 0; i < 8; ++i) s = fmaf(v[i], g[o][i], s);
#pragma unroll
            for (int x = 1; x < LPH; x <<= 1) s += __shfl_xor(s, x, 64);     // every lane of the head ends with the same sum
            acc[o] = s;
        }
        if (valid) {
            const float scale = p.scale[n];
            float* out = p.out + (ro * C + (int64_t)l * p.H + h) * p.O;
            // column o is stored by the head's lane o % LPH (lanes past d_head / 8 are not `valid`: lane 0 takes theirs)
            const int nc = (p.dh + 7) / 8;
#pragma unroll
            for (int o = 0; o < OC; ++o) {
                const int owner = (o & (LPH - 1)) < nc ? (o & (LPH - 1)) : 0;
                if (o < p.O && c == owner) {
                    const float s = acc[o];
                    out[o] = (fabsf(s) <= 3.402823466e38f) ? __fdiv_rn(s, scale) : __uint_as_float(0x7fc00000u);
                }
            }
        }
    }
}

template <int LPH>
void attr_launch_head(const AttrHeadParams& p, dim3 grid, hipStream_t stream) {
    if (p.O == 1) hipLaunchKernelGGL((attr_head_kernel<LPH, 1>), grid, dim3(256), 0, stream, p);
    else if (p.O <= 4) hipLaunchKernelGGL((attr_head_kernel<LPH, 4>), grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((attr_head_kernel<LPH, 16>), grid, dim3(256), 0, stream, p);
}

bool attr_d_head_served(int d_head) {
    return d_head == 32 || d_head == 64 || (d_head > 64 && d_head <= 128 && d_head % 8 == 0);
}

}  // namespace

int attr_launch_fold(const char* who, const void* const* W, int n_layers, int64_t HD, int d_model, int64_t R, const float* answers,
                     float* G, hipStream_t stream) {
    AttrPtrs w{};
    for (int l = 0; l < n_layers; ++l) w.ptr[l] = W[l];
    const int64_t r_tiles = (R + FOLD_TR - 1) / FOLD_TR;
    PV_REQUIRE(r_tiles <= 65535, std::string(who) + ": more than 65535 * 16 answer rows in one call");
    const dim3 grid((unsigned)((HD + FOLD_TJ - 1) / FOLD_TJ), (unsigned)r_tiles, (unsigned)n_layers);
    hipLaunchKernelGGL(attr_fold_kernel, grid, dim3(256), 0, stream, w, answers, (int)HD, d_model, (int)R, G);
    PV_LAUNCH_CHECK("attr_fold_kernel");
    return PV_OK;
}

extern "C" size_t pv_head_attribution_workspace_bytes(int32_t n_layers, int32_t n_heads, int32_t d_head, int32_t n_answer_rows) {
    if (n_layers <= 0 || n_heads <= 0 || d_head <= 0 || n_answer_rows <= 0) return 0;
    return (size_t)pv_align_up((int64_t)n_layers * n_answer_rows * n_heads * d_head * 4, 256);
}

extern "C" int pv_head_attribution(int32_t dtype, const void* const* z, const void* const* W_O, int32_t n_layers, int32_t n_images,
                                   int32_t n_tokens, int32_t pos, int32_t n_heads, int32_t d_head, int32_t d_model,
                                   const float* scale, const float* answers, int32_t n_answers, int32_t per_image, float* out,
                                   void* workspace, size_t workspace_bytes, void* stream_) {
    PV_REQUIRE(dtype == PV_DTYPE_BF16, "head attribution: the taps and W_O must be bf16 (dtype PV_DTYPE_BF16); fp32 is not served");
    PV_REQUIRE(attr_d_head_served(d_head), "head attribution: d_head must be 32, 64, or a multiple of 8 in (64, 128]");
    PV_REQUIRE(d_model >= 8 && d_model % 8 == 0, "head attribution: d_model must be a multiple of 8 (16-byte operand chunks)");
    PV_REQUIRE(n_layers >= 1 && n_layers <= PV_ATTR_MAX_LAYERS,
               "head attribution: n_layers must be between 1 and PV_ATTR_MAX_LAYERS = " PV_STR(PV_ATTR_MAX_LAYERS));
    PV_REQUIRE(n_answers >= 1 && n_answers <= PV_ATTR_MAX_ANSWERS,
               "head attribution: n_answers must be between 1 and PV_ATTR_MAX_ANSWERS = " PV_STR(PV_ATTR_MAX_ANSWERS));
    PV_REQUIRE(n_images >= 1 && n_tokens >= 1 && n_heads >= 1, "head attribution: n_images, n_tokens and n_heads must be positive");
    PV_REQUIRE(pos >= -1 && pos < n_tokens, "head attribution: pos must be -1 (every token) or a token index below n_tokens");
    PV_REQUIRE(z && W_O && scale && answers && out && workspace,
               "head attribution: z, W_O, scale, answers, out and workspace must not be NULL");
    PV_REQUIRE(pv_aligned16(answers) && pv_aligned16(workspace), "head attribution: answers and workspace must be 16-byte aligned");
    for (int l = 0; l < n_layers; ++l)
        PV_REQUIRE(z[l] && W_O[l] && pv_aligned16(z[l]) && pv_aligned16(W_O[l]),
                   "head attribution: every tap and every W_O must be a 16-byte aligned device pointer");
    const int64_t HD = (int64_t)n_heads * d_head;
    PV_REQUIRE((uint64_t)n_images * (uint64_t)n_tokens * (uint64_t)HD * 2 < (1ull << 32),
               "head attribution: a tap must stay below 4 GiB");
    const int64_t R = per_image ? (int64_t)n_images * n_answers : n_answers;
    PV_REQUIRE(HD < (1 << 24) && R < (1 << 30), "head attribution: n_heads * d_head or the number of answer rows is out of range");
    const size_t need = pv_head_attribution_workspace_bytes(n_layers, n_heads, d_head, (int32_t)R);
    if (workspace_bytes < need) {
        pv_set_error("head attribution: workspace too small (pv_head_attribution_workspace_bytes)");
        return PV_ERR_WORKSPACE;
    }
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    float* G = reinterpret_cast<float*>(workspace);

    if (const int rc = attr_launch_fold("head attribution", W_O, n_layers, HD, d_model, R, answers, G, stream)) return rc;

    AttrHeadParams p{};
    for (int l = 0; l < n_layers; ++l) p.z.ptr[l] = z[l];
    p.G = G; p.scale = scale; p.out = out;
    p.H = n_heads; p.dh = d_head; p.L = n_layers; p.O = n_answers; p.R = (int32_t)R;
    p.T = n_tokens; p.pos = pos;
    const int t_out = pos < 0 ? n_tokens : 1;
    p.per_image = per_image ? 1 : 0;
    p.n_seg = per_image ? n_images : 1;
    p.seg_rows = per_image ? t_out : n_images * t_out;
    const int lph = d_head == 32 ? 4 : d_head == 64 ? 8 : 16;
    p.HG = n_heads < 256 / lph ? n_heads : 256 / lph;
    p.n_hg = (n_heads + p.HG - 1) / p.HG;
    p.RP = 256 / (p.HG * lph);
    p.passes = (32 + p.RP - 1) / p.RP;                       // tiles of about 32 rows: G is fetched once per tile
    const int tile_rows = p.RP * p.passes;
    p.n_tile = (p.seg_rows + tile_rows - 1) / tile_rows;
    const int64_t blocks = (int64_t)n_layers * p.n_seg * p.n_tile * p.n_hg;
    PV_REQUIRE(blocks < (1ll << 31), "head attribution: the launch would need 2^31 workgroups or more");
    const dim3 grid((unsigned)blocks);
    if (lph == 4) attr_launch_head<4>(p, grid, stream);
    else if (lph == 8) attr_launch_head<8>(p, grid, stream);
    else attr_launch_head<16>(p, grid, stream);
    PV_LAUNCH_CHECK("attr_head_kernel");
    return PV_OK;
}
