// gemm_kernel: the GEMM for whatever the DMA kernels do not take (index of the GEMM files: gemm.hip).  128 x 128 tile, 256 threads,
// operands staged through registers into padded LDS rows, double-buffered.  Both dtypes, any alignment, patch gather, [K][N] B operand.
//   K in slabs of 128 BYTES per row, LDS rows of 144 bytes: 9 r mod 16 is a permutation over a 16-lane service group, so the
//   ds_read_b128 fragment reads are conflict-free; lane l reads row l & 31, chunk 2 j + (l >> 5): for bf16 that IS the
//   v_mfma_f32_32x32x16_bf16 operand, for fp32 the 4 floats feed 4 v_mfma_f32_32x32x2_f32.
// Also here: act_rows_kernel (pv_launch_act), the activation of the GEMM epilogues over rows already stored.
#include "gemm_epi.hpp"

namespace {

constexpr int SLAB = 128;            // bytes of K per row per stage
constexpr int ROWB = 144;            // padded LDS row (bytes)
constexpr int TILE_BYTES = BM * ROWB;   // 18432
constexpr int CS_LD = 68;            // fp32 staging row (floats): 64 + 4 pad
constexpr int GEMM_LDS = 4 * TILE_BYTES;   // As[2] + Bs[2] = 73728 >= 4 waves * 64*68*4 = 69632

template <typename T, int AMODE, bool VEC>
struct Loader {
    // one 16-byte chunk of operand A for global row gm at K byte offset kb
    __device__ static __forceinline__ uint4 load_a(const GemmParams& p, int gm, int kb) {
        constexpr int EB = DT<T>::kBytes;
        constexpr int PC = DT<T>::kPerChunk;
        const int Kb = p.K * EB;
        uint4 z = make_uint4(0, 0, 0, 0);
        if (gm >= p.M || kb >= Kb) return z;
        const unsigned char* base = reinterpret_cast<const unsigned char*>(p.A);
        if constexpr (AMODE == PV_A_PLAIN) {
            const unsigned char* ptr = base + (int64_t)gm * p.lda * EB + kb;
            if constexpr (VEC) {
                return *reinterpret_cast<const uint4*>(ptr);
            } else {
                alignas(16) T tmp[PC];
                const T* e = reinterpret_cast<const T*>(ptr);
                const int ke = kb / EB;
#pragma unroll
                for (int i = 0; i < PC; ++i) tmp[i] = (ke + i < p.K) ? e[i] : T(0);
                return *reinterpret_cast<uint4*>(tmp);
            }
        } else {
            // im2col-free patch gather: row gm = (image b, patch py, px); k = (c, i, j)
            const int np = p.pG * p.pG;
            const int b = gm / np, pidx = gm - b * np;
            const int py = pidx / p.pG, px = pidx - py * p.pG;
            const int pp = p.pP * p.pP;
            const int ke = kb / EB;
            if constexpr (VEC) {
                const int c = ke / pp, rem = ke - c * pp;
                const int i = rem / p.pP, j = rem - i * p.pP;
                const int64_t off = (((int64_t)b * p.pC + c) * p.pS + (py * p.pP + i)) * p.pS + px * p.pP + j;
                return *reinterpret_cast<const uint4*>(base + off * EB);
            } else {
                alignas(16) T tmp[PC];
#pragma unroll
                for (int t = 0; t < PC; ++t) {
                    const int k = ke + t;
                    if (k < p.K) {
                        const int c = k / pp, rem = k - c * pp;
                        const int i = rem / p.pP, j = rem - i * p.pP;
                        const int64_t off = (((int64_t)b * p.pC + c) * p.pS + (py * p.pP + i)) * p.pS + px * p.pP + j;
                        tmp[t] = reinterpret_cast<const T*>(base)[off];
                    } else {
                        tmp[t] = T(0);
                    }
                }
                return *reinterpret_cast<uint4*>(tmp);
            }
        }
    }
    __device__ static __forceinline__ uint4 load_b(const GemmParams& p, int gn, int kb) {
        constexpr int EB = DT<T>::kBytes;
        constexpr int PC = DT<T>::kPerChunk;
        const int Kb = p.K * EB;
        if (gn >= p.N || kb >= Kb) return make_uint4(0, 0, 0, 0);
        const unsigned char* ptr = reinterpret_cast<const unsigned char*>(p.Bt) + (int64_t)gn * p.ldb * EB + kb;
        if constexpr (VEC) {
            return *reinterpret_cast<const uint4*>(ptr);
        } else {
            alignas(16) T tmp[PC];
            const T* e = reinterpret_cast<const T*>(ptr);
            const int ke = kb / EB;
#pragma unroll
            for (int i = 0; i < PC; ++i) tmp[i] = (ke + i < p.K) ? e[i] : T(0);
            return *reinterpret_cast<uint4*>(tmp);
        }
    }
};

// accumulators -> per-wave LDS staging (reusing the operand buffers; caller has passed a barrier after
// the last LDS read) -> each lane owns 8 consecutive columns of a row -> fused epilogue + tap stores
template <typename T>
__device__ __forceinline__ void tile_epilogue(const GemmParams& p, f32x16 (&acc)[2][2], unsigned char* smem, int m0, int n0,
                                              int wave, int lane, int wm, int wn) {
    float* Cs = reinterpret_cast<float*>(smem) + wave * (64 * CS_LD);
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
                const int col = ni * 32 + (lane & 31);
                Cs[row * CS_LD + col] = acc[mi][ni][e];
            }
    __syncthreads();
#pragma unroll 2
    for (int it = 0; it < 8; ++it) {
        const int row = it * 8 + (lane >> 3);
        const int cc = (lane & 7) * 8;
        const int gm = m0 + wm * 64 + row;
        const int gn = n0 + wn * 64 + cc;
        if (gm < p.M && gn < p.N) {
            float v[8];
            const float4 x0 = *reinterpret_cast<const float4*>(Cs + row * CS_LD + cc);
            const float4 x1 = *reinterpret_cast<const float4*>(Cs + row * CS_LD + cc + 4);
            v[0] = x0.x; v[1] = x0.y; v[2] = x0.z; v[3] = x0.w;
            v[4] = x1.x; v[5] = x1.y; v[6] = x1.z; v[7] = x1.w;
            epilogue8<T>(p, v, gm, gn);
        }
    }
}

constexpr int BKN_ROW = 528;         // [K][N]-layout B tile: 128 floats + 16 pad bytes per k row

template <typename T, int AMODE, bool VEC, bool BKN = false>
__global__ __launch_bounds__(256, 2) void gemm_kernel(const GemmParams p) {
    static_assert(!BKN || sizeof(T) == 4, "[K][N] B operand is fp32 only");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* As = smem;                      // [2][TILE_BYTES]
    unsigned char* Bs = smem + 2 * TILE_BYTES;     // [2][TILE_BYTES]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;

    // XCD-aware, bijective remap of the linear workgroup id (block b runs on XCD b % 8): each XCD
    // gets a contiguous run of tiles; tiles are ordered N-fastest so a run shares A rows.
    const int swz = kloop::xcd_run(blockIdx.x, gridDim.x);
    const int ntn = (p.N + BN - 1) / BN;
    const int tile_m = swz / ntn, tile_n = swz - tile_m * ntn;
    const int m0 = tile_m * BM, n0 = tile_n * BN;

    constexpr int EB = DT<T>::kBytes;
    const int Kb = p.K * EB;
    const int nk = (Kb + SLAB - 1) / SLAB;

    // staging assignment: chunk c = tid + 256*i -> row c >> 3, 16-byte column c & 7
    uint4 ra[4], rb[4];
    auto load_slab = [&](int kt) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = tid + 256 * i;
            const int row = c >> 3, kc = c & 7;
            const int kb = kt * SLAB + kc * 16;
            ra[i] = Loader<T, AMODE, VEC>::load_a(p, m0 + row, kb);
            if constexpr (BKN) {
                // B[k][n]: chunk c -> k row c >> 5 (32 per slab), 4-float column group c & 31
                const int krow = kt * 32 + (c >> 5), nn = n0 + (c & 31) * 4;
                rb[i] = (krow < p.K && nn < p.N)
                            ? *reinterpret_cast<const uint4*>(reinterpret_cast<const float*>(p.Bt) + (int64_t)krow * p.ldb + nn)
                            : make_uint4(0, 0, 0, 0);
            } else {
                rb[i] = Loader<T, AMODE, VEC>::load_b(p, n0 + row, kb);
            }
        }
    };
    auto store_slab = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = tid + 256 * i;
            const int row = c >> 3, kc = c & 7;
            *reinterpret_cast<uint4*>(As + buf * TILE_BYTES + row * ROWB + kc * 16) = ra[i];
            if constexpr (BKN)
                *reinterpret_cast<uint4*>(Bs + buf * TILE_BYTES + (c >> 5) * BKN_ROW + (c & 31) * 16) = rb[i];
            else
                *reinterpret_cast<uint4*>(Bs + buf * TILE_BYTES + row * ROWB + kc * 16) = rb[i];
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

    const int a_off = (wm * 64 + (lane & 31)) * ROWB + (lane >> 5) * 16;
    const int b_off = (wn * 64 + (lane & 31)) * ROWB + (lane >> 5) * 16;

    load_slab(0);
    store_slab(0);
    __syncthreads();

    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) load_slab(kt + 1);
        const unsigned char* Ab = As + buf * TILE_BYTES;
        const unsigned char* Bb = Bs + buf * TILE_BYTES;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint4 a[2], b[2];
            a[0] = *reinterpret_cast<const uint4*>(Ab + a_off + j * 32);
            a[1] = *reinterpret_cast<const uint4*>(Ab + a_off + 32 * ROWB + j * 32);
            if constexpr (BKN) {
                // MFMA step (j, e) consumes k = 8 j + 4 (lane >> 5) + e on the A side; fetch the same k
                const float* bk = reinterpret_cast<const float*>(Bb + (8 * j + 4 * (lane >> 5)) * BKN_ROW) + wn * 64 + (lane & 31);
                b[0] = make_uint4(__float_as_uint(bk[0]), __float_as_uint(bk[BKN_ROW / 4]),
                                  __float_as_uint(bk[2 * (BKN_ROW / 4)]), __float_as_uint(bk[3 * (BKN_ROW / 4)]));
                b[1] = make_uint4(__float_as_uint(bk[32]), __float_as_uint(bk[BKN_ROW / 4 + 32]),
                                  __float_as_uint(bk[2 * (BKN_ROW / 4) + 32]), __float_as_uint(bk[3 * (BKN_ROW / 4) + 32]));
            } else {
                b[0] = *reinterpret_cast<const uint4*>(Bb + b_off + j * 32);
                b[1] = *reinterpret_cast<const uint4*>(Bb + b_off + 32 * ROWB + j * 32);
            }
            if constexpr (EB == 2) {
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni)
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                            __builtin_bit_cast(bf16x8, a[mi]), __builtin_bit_cast(bf16x8, b[ni]),
                            acc[mi][ni], 0, 0, 0);
            } else {
                const float af[2][4] = {{__uint_as_float(a[0].x), __uint_as_float(a[0].y),
                                         __uint_as_float(a[0].z), __uint_as_float(a[0].w)},
                                        {__uint_as_float(a[1].x), __uint_as_float(a[1].y),
                                         __uint_as_float(a[1].z), __uint_as_float(a[1].w)}};
                const float bf[2][4] = {{__uint_as_float(b[0].x), __uint_as_float(b[0].y),
                                         __uint_as_float(b[0].z), __uint_as_float(b[0].w)},
                                        {__uint_as_float(b[1].x), __uint_as_float(b[1].y),
                                         __uint_as_float(b[1].z), __uint_as_float(b[1].w)}};
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                        for (int ni = 0; ni < 2; ++ni)
                            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(
                                af[mi][e], bf[ni][e], acc[mi][ni], 0, 0, 0);
            }
        }
        if (kt + 1 < nk) store_slab(buf ^ 1);
        __syncthreads();
    }

    tile_epilogue<T>(p, acc, smem, m0, n0, wave, lane, wm, wn);
}

template <typename T, int AMODE, bool VEC, bool BKN = false>
int launch(const GemmParams& p, const GemmChoice& c, hipStream_t stream) {
    static bool attr_done = false;
    if (!attr_done) {
        PV_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_kernel<T, AMODE, VEC, BKN>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, GEMM_LDS));
        attr_done = true;
    }
    {
        const GemmCost cost = gemm_cost<T>(p);
        ProfScope prof(PV_PROF_GEMM, stream, cost.flops, cost.bytes);
        hipLaunchKernelGGL((gemm_kernel<T, AMODE, VEC, BKN>), dim3(c.grid), dim3(256), GEMM_LDS, stream, p);
    }
    PV_LAUNCH_CHECK("gemm_kernel");
    return PV_OK;
}

// the four (operand mode, vector loads) forms of one dtype
template <typename T>
int launch_any(const GemmParams& p, const GemmChoice& c, hipStream_t stream) {
    if (p.a_mode == PV_A_PLAIN) {
        return c.vec ? launch<T, PV_A_PLAIN, true>(p, c, stream) : launch<T, PV_A_PLAIN, false>(p, c, stream);
    }
    return c.vec ? launch<T, PV_A_PATCH, true>(p, c, stream) : launch<T, PV_A_PATCH, false>(p, c, stream);
}

template <typename T>
__global__ __launch_bounds__(256) void act_rows_kernel(const T* __restrict__ pre, T* __restrict__ post, int64_t n8, int act) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    float v[8];
    load8(pre + i * 8, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = act_any<T>(v[e], act);
    store8(post + i * 8, v);
}

}  // namespace

int pv_gemm_launch_generic(int dtype, const GemmParams& p, const GemmChoice& c, hipStream_t stream) {
    if (p.b_kn) return launch<float, PV_A_PLAIN, true, true>(p, c, stream);
    return dtype == PV_DTYPE_BF16 ? launch_any<bf16_t>(p, c, stream) : launch_any<float>(p, c, stream);
}

int pv_launch_act(int dtype, int act, const void* pre, void* post, int64_t n, hipStream_t stream) {
    PV_REQUIRE(pre && post && n > 0 && n % 8 == 0 && pv_aligned16(pre) && pv_aligned16(post), "activation launcher arguments");
    const int64_t n8 = n / 8;
    const dim3 grid((unsigned)((n8 + 255) / 256)), block(256);
    if (dtype == PV_DTYPE_BF16)
        hipLaunchKernelGGL(act_rows_kernel<bf16_t>, grid, block, 0, stream, reinterpret_cast<const bf16_t*>(pre), reinterpret_cast<bf16_t*>(post), n8, act);
    else
        hipLaunchKernelGGL(act_rows_kernel<float>, grid, block, 0, stream, reinterpret_cast<const float*>(pre), reinterpret_cast<float*>(post), n8, act);
    PV_LAUNCH_CHECK("act_rows_kernel");
    return PV_OK;
}
