// The GEMM of the dense SAE steps (gfx950; the five GEMMs of a step: sae_dense.hip): the exact fp32 matrix instruction or the split-fp16
// form, a step's elementwise work in the epilogues (DenseGemm); the operand maxima of the split form; the sums of the column partials.
#include "kloop.hpp"
#include "sae_dense_gemm.hpp"

namespace {

constexpr int DG_BM = 128, DG_BN = 128;
constexpr int DG_ROWB = 144;                  // K-contiguous tile: 128 rows x (128 + 16 pad) bytes
constexpr int DG_KROW = 528;                  // row-contiguous tile: 32 k-rows x (512 + 16 pad) bytes
constexpr int DG_TILE = DG_BM * DG_ROWB;      // 18432 >= 32 * 528
constexpr int DG_CS_LD = 68;                  // fp32 staging row of the epilogue (floats)
constexpr int DG_LDS = 4 * DG_TILE;           // As[2] + Bs[2] = 73728 >= 4 waves x 64 x 68 x 4

// 16 bytes from global memory, or zeros (a plain branch: `ok ? *p : zero` makes hipcc select between two ADDRESSES and park the
// staging registers in scratch)
__device__ __forceinline__ uint4 ld16_or_zero(const float* ptr, bool ok) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (ok) v = *reinterpret_cast<const uint4*>(ptr);
    return v;
}

// ---- the split-fp16 K loop (round 6) ------------------------------------------------------------------------------------------
// The fp32 matrix instruction runs at 1/16 of the fp16 one.  An fp32 value x scaled by a power of two s splits EXACTLY into
// s x = hi + lo + r with hi = fp16(s x), lo = fp16(s x - hi) and |r| <= 2^-20 |s x| (both conversions round toward zero:
// v_cvt_pkrtz_f16_f32, one instruction per pair), so a . b = (a_hi b_hi + a_hi b_lo + a_lo b_hi) / (s_a s_b) up to 2^-19 relative per
// product: three fp16 products with fp32 accumulation instead of one fp32 product -- the same tiles and epilogues at 16 / 3 of the
// matrix rate.  s = 2^(13 - floor(log2 max|.|)) per TENSOR (DenseGemm.a_max / b_max: the producers track the maxima), so the largest
// entry lands in [2^13, 2^14) and every entry within 2^-14 of it keeps 21+ bits (smaller ones lose relative, not absolute,
// accuracy: their lo part goes denormal at 2^-24 of the scaled range).  Conversion happens in the staging pass the fp32 kernel has
// anyway (global -> registers -> LDS); the LDS image of an operand is two planes (hi, lo) of [128 rows][32 k] halves -- 64-byte rows,
// 16-byte chunk c of row r at c ^ ((r >> 2) & 3): conflict-free ds_read_b128 fragments, the filter GEMM's image -- whichever of
// its two row-major layouts the fp32 matrix lies in: K-contiguous rows are converted four k at a time, row-contiguous k-slices are
// transposed on the way (a lane loads the same four rows at four consecutive k and writes four 8-byte row pieces).
typedef _Float16 dg_f16x8 __attribute__((ext_vector_type(8)));
constexpr int DG_SPL_PLANE = 128 * 64;          // one operand plane of a stage
constexpr int DG_SPL_STAGE = 4 * DG_SPL_PLANE;  // A hi, A lo, B hi, B lo

// power-of-two scale of an operand from its tracked maximum (bit pattern of max|.|): the largest entry lands in [2^13, 2^14)
__device__ __forceinline__ void dg_scale_of(uint32_t max_bits, float& s, float& inv) {
    int e = (int)((max_bits >> 23) & 0xffu);
    e = e < 24 ? 24 : (e > 250 ? 250 : e);      // (zeros / denormal maxima: any scale is exact on them)
    s = __uint_as_float((uint32_t)(267 - e) << 23);
    inv = __uint_as_float((uint32_t)(e - 13) << 23);
}

// hi / lo halves of four scaled floats, packed as (k0 k1), (k2 k3)
// (both conversions round toward zero, v_cvt_pkrtz_f16_f32: one full-rate instruction per pair.  The round-to-nearest pair
// conversion of gfx950, v_cvt_pk_f16_f32 (-DPV_SPLIT_RNE), is 8 x more accurate per element and was measured 2.1 ms per step slower
// -- 6.02 against 3.90 ms for the ReLU + L1 step, profiles/r06_dense_split_fp16_ab.txt -- while the product's error is already below
// that of an fp32 accumulation either way: a numpy emulation over K = 768 gives 3.4e-7 of the largest entry for this form, 6e-8 for
// round-to-nearest, 6.2e-7 for numpy's own fp32 matmul.)
__device__ __forceinline__ void dg_split4(float x0, float x1, float x2, float x3, float s, uint2& hi, uint2& lo) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    typedef float f2 __attribute__((ext_vector_type(2)));
    const f2 a = {x0 * s, x1 * s}, b = {x2 * s, x3 * s};
#ifndef PV_SPLIT_RNE
    typedef __fp16 hz2 __attribute__((ext_vector_type(2)));
    const hz2 z01 = __builtin_amdgcn_cvt_pkrtz(a[0], a[1]), z23 = __builtin_amdgcn_cvt_pkrtz(b[0], b[1]);
    const hz2 y01 = __builtin_amdgcn_cvt_pkrtz(a[0] - (float)z01[0], a[1] - (float)z01[1]);
    const hz2 y23 = __builtin_amdgcn_cvt_pkrtz(b[0] - (float)z23[0], b[1] - (float)z23[1]);
    const h2 h01 = __builtin_bit_cast(h2, z01), h23 = __builtin_bit_cast(h2, z23), l01 = __builtin_bit_cast(h2, y01), l23 = __builtin_bit_cast(h2, y23);
#else
    const h2 h01 = __builtin_convertvector(a, h2), h23 = __builtin_convertvector(b, h2);
    const h2 l01 = __builtin_convertvector(a - __builtin_convertvector(h01, f2), h2);
    const h2 l23 = __builtin_convertvector(b - __builtin_convertvector(h23, f2), h2);
#endif
    hi = make_uint2(__builtin_bit_cast(uint32_t, h01), __builtin_bit_cast(uint32_t, h23));
    lo = make_uint2(__builtin_bit_cast(uint32_t, l01), __builtin_bit_cast(uint32_t, l23));
}

template <bool A_KM, bool B_KN, int EPI_, bool SPLIT = false>
__global__ __launch_bounds__(256, 2) void dense_gemm_kernel(const DenseGemm p) {
    // (the tail variants are their own instantiations: tanhf / powf inlined into the plain ENC / DH epilogues cost the split-fp16 step
    // 2.2 ms of 3.8 although never executed there)
    constexpr bool TAIL = EPI_ == DG_EPI_ENC_T || EPI_ == DG_EPI_DH_T;
    constexpr int EPI = EPI_ == DG_EPI_ENC_T ? DG_EPI_ENC : (EPI_ == DG_EPI_DH_T ? DG_EPI_DH : EPI_);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (p.gate && *p.gate != 1u) return;                   // (uniform over the grid)
    unsigned char* As = smem;
    unsigned char* Bs = smem + 2 * DG_TILE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    // XCD-aware bijective remap (block b runs on XCD b % 8): each XCD gets a contiguous run of tiles, N fastest
    const int swz = kloop::xcd_run(blockIdx.x, gridDim.x);
    const int ntn = (p.N + DG_BN - 1) / DG_BN;
    // Tile order inside an XCD's run.  N fastest (group 0) lets the 64 tiles an XCD runs at a time share ONE row slab and stream 64
    // different column slabs: at a wide output (the encoder and dH GEMMs: 192 column tiles of 393 KB operand rows each) every XCD
    // drags the whole B matrix through its 4 MB L2 once per row tile -- 2.8 GB of HBM fetches for a 75 MB matrix, PMC-measured, and
    // the kernel was bound by them.  Grouped (group G > 0): G row tiles x all column tiles per group, the row tile fastest inside --
    // the G tiles that share a column slab run side by side, the slab is fetched once per group.
    int tile_m, tile_n;
    if (p.group > 0) {
        const int ntm = (p.M + DG_BM - 1) / DG_BM;
        const int per = p.group * ntn, g = swz / per, idx = swz - g * per;
        const int gc = min(p.group, ntm - g * p.group);
        tile_n = idx / gc;
        tile_m = g * p.group + (idx - tile_n * gc);
    } else {
        tile_m = swz / ntn;
        tile_n = swz - tile_m * ntn;
    }
    const int m0 = tile_m * DG_BM, n0 = tile_n * DG_BN;
    const int k_begin = blockIdx.y * p.k_chunk, k_end = min(p.K, k_begin + p.k_chunk);
    const int nk = (k_end - k_begin + DG_KSLAB - 1) / DG_KSLAB;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

    const int l31 = lane & 31, half = lane >> 5;
    float inv_a = 1.0f, inv_b = 1.0f;                      // SPLIT: the two inverse operand scales (applied in the epilogue)
    if constexpr (SPLIT) {
        // ---- operand scales: the largest of the tracked partial maxima (one slot per thread)
        float sa, sb;
        {
            uint32_t ma = p.a_max[tid], mb = p.b_max[tid];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                ma = max(ma, (uint32_t)__shfl_xor((int)ma, o, 64));
                mb = max(mb, (uint32_t)__shfl_xor((int)mb, o, 64));
            }
            uint32_t* red = reinterpret_cast<uint32_t*>(smem);
            if (lane == 0) { red[wave] = ma; red[4 + wave] = mb; }
            __syncthreads();
            ma = max(max(red[0], red[1]), max(red[2], red[3]));
            mb = max(max(red[4], red[5]), max(red[6], red[7]));
            __syncthreads();
            dg_scale_of(ma, sa, inv_a);
            dg_scale_of(mb, sb, inv_b);
        }
        uint4 ra[4], rb[4];
        const int rgl = lane & 7, kql = lane >> 3;             // row-contiguous sources: rows wave * 32 + 4 rgl .. + 3 at k = 4 kql + i
        auto load_slab = [&](int kt) {
            const int kb = k_begin + kt * DG_KSLAB;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = tid + 256 * i;
                if constexpr (A_KM) {
                    const int k = kb + 4 * kql + i, mm = m0 + wave * 32 + 4 * rgl;
                    ra[i] = ld16_or_zero(p.A + (int64_t)k * p.lda + mm, k < k_end && mm < p.M);
                } else {
                    const int mm = m0 + (c >> 3), k = kb + (c & 7) * 4;
                    ra[i] = ld16_or_zero(p.A + (int64_t)mm * p.lda + k, mm < p.M && k < k_end);
                }
                if constexpr (B_KN) {
                    const int k = kb + 4 * kql + i, nn = n0 + wave * 32 + 4 * rgl;
                    rb[i] = ld16_or_zero(p.B + (int64_t)k * p.ldb + nn, k < k_end && nn < p.N);
                } else {
                    const int nn = n0 + (c >> 3), k = kb + (c & 7) * 4;
                    rb[i] = ld16_or_zero(p.B + (int64_t)nn * p.ldb + k, nn < p.N && k < k_end);
                }
            }
        };
        auto put = [&](unsigned char* plane_hi, int row, int kgrp, float x0, float x1, float x2, float x3, float sc) {
            uint2 hi, lo;
#if defined(PV_DG_NOCVT)
            hi = make_uint2(__float_as_uint(x0), __float_as_uint(x1)); lo = make_uint2(__float_as_uint(x2), __float_as_uint(x3));
#elif defined(PV_DG_HALFCVT)                           // (timing ablation: the hi halves only -- 2^-11 products, the step stays dense)
            {
                typedef __fp16 hz2 __attribute__((ext_vector_type(2)));
                const hz2 z01 = __builtin_amdgcn_cvt_pkrtz(x0 * sc, x1 * sc), z23 = __builtin_amdgcn_cvt_pkrtz(x2 * sc, x3 * sc);
                hi = make_uint2(__builtin_bit_cast(uint32_t, z01), __builtin_bit_cast(uint32_t, z23));
                lo = make_uint2(0u, 0u);
            }
#else
            dg_split4(x0, x1, x2, x3, sc, hi, lo);
#endif
            const int off = row * 64 + ((((kgrp >> 1) ^ (row >> 2)) & 3) << 4) + (kgrp & 1) * 8;
            *reinterpret_cast<uint2*>(plane_hi + off) = hi;
            *reinterpret_cast<uint2*>(plane_hi + DG_SPL_PLANE + off) = lo;
        };
        auto store_operand = [&](unsigned char* plane_hi, const uint4 (&r)[4], bool km, float sc) {
            if (km) {
                const int row = wave * 32 + 4 * rgl;
                put(plane_hi, row + 0, kql, __uint_as_float(r[0].x), __uint_as_float(r[1].x), __uint_as_float(r[2].x), __uint_as_float(r[3].x), sc);
                put(plane_hi, row + 1, kql, __uint_as_float(r[0].y), __uint_as_float(r[1].y), __uint_as_float(r[2].y), __uint_as_float(r[3].y), sc);
                put(plane_hi, row + 2, kql, __uint_as_float(r[0].z), __uint_as_float(r[1].z), __uint_as_float(r[2].z), __uint_as_float(r[3].z), sc);
                put(plane_hi, row + 3, kql, __uint_as_float(r[0].w), __uint_as_float(r[1].w), __uint_as_float(r[2].w), __uint_as_float(r[3].w), sc);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int c = tid + 256 * i;
                    put(plane_hi, c >> 3, c & 7, __uint_as_float(r[i].x), __uint_as_float(r[i].y), __uint_as_float(r[i].z), __uint_as_float(r[i].w), sc);
                }
            }
        };
        auto store_slab = [&](int buf) {
            store_operand(smem + buf * DG_SPL_STAGE, ra, A_KM, sa);
            store_operand(smem + buf * DG_SPL_STAGE + 2 * DG_SPL_PLANE, rb, B_KN, sb);
        };
        if (nk > 0) {
            load_slab(0);
            store_slab(0);
        }
        __syncthreads();
        const int sw = kloop::swz64(l31);
        for (int kt = 0; kt < nk; ++kt) {
            const int buf = kt & 1;
#ifndef PV_DG_NOLOAD                                   // (timing ablations of tools/build_variant.sh builds: results are wrong with any of them)
            if (kt + 1 < nk) load_slab(kt + 1);
#endif
            const unsigned char* Ab = smem + buf * DG_SPL_STAGE;
            const unsigned char* Bb = Ab + 2 * DG_SPL_PLANE;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int co = ((ks * 2 + half) ^ sw) << 4;
                dg_f16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) {
                    const unsigned char* a = Ab + (wm * 64 + mi * 32 + l31) * 64 + co;
                    ah[mi] = __builtin_bit_cast(dg_f16x8, *reinterpret_cast<const uint4*>(a));
                    al[mi] = __builtin_bit_cast(dg_f16x8, *reinterpret_cast<const uint4*>(a + DG_SPL_PLANE));
                }
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) {
                    const unsigned char* b = Bb + (wn * 64 + ni * 32 + l31) * 64 + co;
                    bh[ni] = __builtin_bit_cast(dg_f16x8, *reinterpret_cast<const uint4*>(b));
                    bl[ni] = __builtin_bit_cast(dg_f16x8, *reinterpret_cast<const uint4*>(b + DG_SPL_PLANE));
                }
#ifndef PV_DG_NOMFMA
                // (the two cross terms first: they are 2^-11 of the main term)
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[mi], bh[ni], acc[mi][ni], 0, 0, 0);
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[mi], bl[ni], acc[mi][ni], 0, 0, 0);
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[mi], bh[ni], acc[mi][ni], 0, 0, 0);
#else
                acc[0][0][0] += (float)ah[0][0] + (float)al[1][1] + (float)bh[0][2] + (float)bl[1][3] + (float)ah[1][4] + (float)al[0][5] + (float)bh[1][6] + (float)bl[0][7];
#endif
            }
            if (kt + 1 < nk) store_slab(buf ^ 1);
            __syncthreads();
        }
    } else {
        uint4 ra[4], rb[4];
        auto load_slab = [&](int kt) {
            const int kb = k_begin + kt * DG_KSLAB;
    #pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = tid + 256 * i;
                if constexpr (A_KM) {                      // chunk c -> k row c >> 5, 4-float group c & 31 of the 128 rows
                    const int k = kb + (c >> 5), mm = m0 + (c & 31) * 4;
                    ra[i] = ld16_or_zero(p.A + (int64_t)k * p.lda + mm, k < k_end && mm < p.M);
                } else {                                   // chunk c -> row c >> 3, 4-float k group c & 7
                    const int mm = m0 + (c >> 3), k = kb + (c & 7) * 4;
                    ra[i] = ld16_or_zero(p.A + (int64_t)mm * p.lda + k, mm < p.M && k < k_end);
                }
                if constexpr (B_KN) {
                    const int k = kb + (c >> 5), nn = n0 + (c & 31) * 4;
                    rb[i] = ld16_or_zero(p.B + (int64_t)k * p.ldb + nn, k < k_end && nn < p.N);
                } else {
                    const int nn = n0 + (c >> 3), k = kb + (c & 7) * 4;
                    rb[i] = ld16_or_zero(p.B + (int64_t)nn * p.ldb + k, nn < p.N && k < k_end);
                }
            }
        };
        auto store_slab = [&](int buf) {
    #pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = tid + 256 * i;
                if constexpr (A_KM) *reinterpret_cast<uint4*>(As + buf * DG_TILE + (c >> 5) * DG_KROW + (c & 31) * 16) = ra[i];
                else *reinterpret_cast<uint4*>(As + buf * DG_TILE + (c >> 3) * DG_ROWB + (c & 7) * 16) = ra[i];
                if constexpr (B_KN) *reinterpret_cast<uint4*>(Bs + buf * DG_TILE + (c >> 5) * DG_KROW + (c & 31) * 16) = rb[i];
                else *reinterpret_cast<uint4*>(Bs + buf * DG_TILE + (c >> 3) * DG_ROWB + (c & 7) * 16) = rb[i];
            }
        };

        if (nk > 0) {
            load_slab(0);
            store_slab(0);
        }
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            const int buf = kt & 1;
            if (kt + 1 < nk) load_slab(kt + 1);
            const unsigned char* Ab = As + buf * DG_TILE;
            const unsigned char* Bb = Bs + buf * DG_TILE;
    #pragma unroll
            for (int j = 0; j < 4; ++j) {
                // MFMA step (j, e) consumes k = 8 j + 4 half + e of the slab on BOTH operands
                float af[2][4], bf[2][4];
    #pragma unroll
                for (int mi = 0; mi < 2; ++mi) {
                    if constexpr (A_KM) {
                        const float* ak = reinterpret_cast<const float*>(Ab + (8 * j + 4 * half) * DG_KROW) + wm * 64 + mi * 32 + l31;
    #pragma unroll
                        for (int e = 0; e < 4; ++e) af[mi][e] = ak[e * (DG_KROW / 4)];
                    } else {
                        const float4 a = *reinterpret_cast<const float4*>(Ab + (wm * 64 + mi * 32 + l31) * DG_ROWB + half * 16 + j * 32);
                        af[mi][0] = a.x; af[mi][1] = a.y; af[mi][2] = a.z; af[mi][3] = a.w;
                    }
                }
    #pragma unroll
                for (int ni = 0; ni < 2; ++ni) {
                    if constexpr (B_KN) {
                        const float* bk = reinterpret_cast<const float*>(Bb + (8 * j + 4 * half) * DG_KROW) + wn * 64 + ni * 32 + l31;
    #pragma unroll
                        for (int e = 0; e < 4; ++e) bf[ni][e] = bk[e * (DG_KROW / 4)];
                    } else {
                        const float4 b = *reinterpret_cast<const float4*>(Bb + (wn * 64 + ni * 32 + l31) * DG_ROWB + half * 16 + j * 32);
                        bf[ni][0] = b.x; bf[ni][1] = b.y; bf[ni][2] = b.z; bf[ni][3] = b.w;
                    }
                }
    #pragma unroll
                for (int e = 0; e < 4; ++e)
    #pragma unroll
                    for (int mi = 0; mi < 2; ++mi)
    #pragma unroll
                        for (int ni = 0; ni < 2; ++ni)
                            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[mi][e], bf[ni][e], acc[mi][ni], 0, 0, 0);
            }
            if (kt + 1 < nk) store_slab(buf ^ 1);
            __syncthreads();
        }

    }

    // ---- epilogue: accumulators -> per-wave LDS block (the operand buffers are free: barrier above) -> a lane owns 8
    // consecutive columns of a row, 8 rows of the wave's 64 x 64 block
    float* Cs = reinterpret_cast<float*>(smem) + wave * (64 * DG_CS_LD);
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * half;
                Cs[row * DG_CS_LD + ni * 32 + l31] = SPLIT ? acc[mi][ni][e] * inv_a * inv_b : acc[mi][ni][e];
            }
    __builtin_amdgcn_wave_barrier();                      // (wave-private block; a wave's LDS operations execute in order)
    const int cc = (lane & 7) * 8;
    const int gn = n0 + wn * 64 + cc;
    const bool col_ok = gn < p.N;                          // N % 8 == 0 is required by the launcher: a chunk is all or nothing
    float csum[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) csum[i] = 0.f;
    float rsum = 0.f;
    float b8[8];
    if constexpr (EPI == DG_EPI_ENC || EPI == DG_EPI_GENC || EPI == DG_EPI_EXPB) {
#pragma unroll
        for (int i = 0; i < 8; ++i) b8[i] = 0.f;
        if (col_ok) load8(p.bias + gn, b8);
    }
    float csum2[8], bm8[8], er8[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { csum2[i] = 0.f; bm8[i] = 0.f; er8[i] = 1.f; }
    if constexpr (EPI == DG_EPI_GENC) {
        if (col_ok) {
            load8(p.bias2 + gn, bm8);
            load8(p.cscale + gn, er8);
#pragma unroll
            for (int i = 0; i < 8; ++i) er8[i] = expf(er8[i]);
        }
    }
    int dslot[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) dslot[i] = -1;
    if constexpr (EPI == DG_EPI_ENC || EPI == DG_EPI_DH) {
        if (p.dead_slot && col_ok) {
#pragma unroll
            for (int i = 0; i < 8; ++i) dslot[i] = p.dead_slot[gn + i];
        }
    }
    float* outz = p.out + (int64_t)blockIdx.y * p.out_zstride;
    float vmax = 0.f;
#pragma unroll 2
    for (int it = 0; it < 8; ++it) {
        const int row = it * 8 + (lane >> 3);
        const int gm = m0 + wm * 64 + row;
        if (gm < p.M && col_ok) {
            float v[8];
            const float4 x0 = *reinterpret_cast<const float4*>(Cs + row * DG_CS_LD + cc);
            const float4 x1 = *reinterpret_cast<const float4*>(Cs + row * DG_CS_LD + cc + 4);
            v[0] = x0.x; v[1] = x0.y; v[2] = x0.z; v[3] = x0.w; v[4] = x1.x; v[5] = x1.y; v[6] = x1.z; v[7] = x1.w;
            float* o = outz + (int64_t)gm * p.ldo + gn;
            if constexpr (EPI == DG_EPI_ENC) {
                if (p.dead_slot) {                                     // ghost gradients: exp(hidden_pre) of the dead features (sae.py:163)
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const int sl = dslot[i];
                        if (sl >= 0) p.dead_act[(int64_t)gm * p.ldd + sl] = expf(v[i] + b8[i]);       // (the accurate exp: the ghost gradients cancel down to ~1e-9, where the fast exp's 1e-6 is visible)
                    }
                }
                float psum = 0.f;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    v[i] = fmaxf(v[i] + b8[i], 0.f);                   // hidden_pre + b_enc -> ReLU (sae.py:567-577)
                    if constexpr (TAIL) {
                        if (p.act == PV_SAE_ACT_TANH_RELU) v[i] = tanhf(v[i]);      // "tanh-relu" (sae.py:823-830)
                    }
                    csum[i] += v[i] > 0.f ? 1.f : 0.f;                // firing counts (train_sae.py:356-364)
                    rsum += v[i];                                     // ||f||_1 (sae.py:617)
                    if constexpr (TAIL) {
                        if (p.lp_part) psum += v[i] > 0.f ? powf(v[i], p.lp) : 0.f;
                    }
                }
                if constexpr (TAIL) {
                    if (p.lp_part) {                                   // sum of f^p over this row's 64 columns (the 8 lanes that share the row)
                        psum += __shfl_xor(psum, 1, 64);
                        psum += __shfl_xor(psum, 2, 64);
                        psum += __shfl_xor(psum, 4, 64);
                        if ((lane & 7) == 0) p.lp_part[(int64_t)gm * ((p.N + 63) / 64) + tile_n * 2 + wn] = psum;
                    }
                }
            } else if constexpr (EPI == DG_EPI_GENC) {
                float g8[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float gate = v[i] + b8[i];                   // gating pre-activation (sae.py:703-706)
                    const float mag = v[i] * er8[i] + bm8[i];          // sae_in @ (W_enc * exp(r_mag)) + b_mag (:708-712)
                    g8[i] = fmaxf(gate, 0.f);                          // relu(gate): L1 + auxiliary path (:773-778)
                    v[i] = gate > 0.f ? fmaxf(mag, 0.f) : 0.f;         // feature_acts (:714-716)
                    csum[i] += v[i] > 0.f ? 1.f : 0.f;
                    csum2[i] += g8[i];
                    rsum += g8[i];
                }
                if (p.amax_out) {                                      // (out2 shares out's maximum: the two are ONE operand [2N][F] of the GEMMs behind)
#pragma unroll
                    for (int i = 0; i < 8; ++i) vmax = fmaxf(vmax, g8[i]);
                }
                store8(p.out2 + (int64_t)gm * p.ldo + gn, g8);
            } else if constexpr (EPI == DG_EPI_DH) {
                float f8[8];
                load8(o, f8);                                          // the stored activation: the ReLU gate of the backward
                float lpt = 0.f;
                if constexpr (TAIL) lpt = p.lp_tok ? p.lp_tok[gm] : 0.f;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    // d loss / d hidden_pre = (dF + l1 / N) [f > 0]; TAIL, lp > 1: the sparsity term's l1 / N ||f_n||_p^(1 - p) f^(p - 1)
                    // instead of the constant; TAIL, tanh-relu: x d tanh = 1 - f^2
                    float g = v[i] + p.add;
                    if constexpr (TAIL) {
                        if (p.lp_tok) g = v[i] + lpt * powf(f8[i], p.lp - 1.f);
                        if (p.act == PV_SAE_ACT_TANH_RELU) g *= 1.f - f8[i] * f8[i];
                    }
                    v[i] = f8[i] > 0.f ? g : 0.f;
                    if (p.dead_slot && dslot[i] >= 0) v[i] += p.dead_act[(int64_t)gm * p.ldd + dslot[i]];    // + the ghost term (not gated)
                    csum[i] += v[i];                                  // gb_enc
                    csum2[i] += v[i] * f8[i];
                }
            } else if constexpr (EPI == DG_EPI_EXPB) {
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = expf(v[i] + b8[i]);         // exp(hidden_pre) of the dead features (sae.py:163), as DG_EPI_ENC writes it
            } else if constexpr (EPI == DG_EPI_MUL) {
                float m8[8];
                load8(p.mul + (int64_t)gm * p.ldo + gn, m8);
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] *= m8[i];
            }
            if (p.amax_out) {
#pragma unroll
                for (int i = 0; i < 8; ++i) vmax = fmaxf(vmax, fabsf(v[i]));
            }
            store8(o, v);
        }
    }
    if (p.amax_out) {                                      // max |out| of this wave's block -> one of the DG_AMAX_SLOTS partial maxima
        vmax = wave_max(vmax);
        if (lane == 0) atomicMax(p.amax_out + ((blockIdx.x * 4 + wave) & (DG_AMAX_SLOTS - 1)), __float_as_uint(vmax));
    }
    if constexpr (EPI == DG_EPI_ENC || EPI == DG_EPI_DH || EPI == DG_EPI_GENC) {
        // the wave's 64 rows of each column: lanes with equal (lane & 7) hold the same 8 columns
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            csum[i] += __shfl_xor(csum[i], 8, 64);
            csum[i] += __shfl_xor(csum[i], 16, 64);
            csum[i] += __shfl_xor(csum[i], 32, 64);
        }
        const int rblk = tile_m * 2 + wm;
        if (lane < 8 && col_ok && m0 + wm * 64 < p.M) store8(p.colpart + (int64_t)rblk * p.N + gn, csum);
        if (EPI != DG_EPI_ENC && p.colpart2) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                csum2[i] += __shfl_xor(csum2[i], 8, 64);
                csum2[i] += __shfl_xor(csum2[i], 16, 64);
                csum2[i] += __shfl_xor(csum2[i], 32, 64);
            }
            if (lane < 8 && col_ok && m0 + wm * 64 < p.M) store8(p.colpart2 + (int64_t)rblk * p.N + gn, csum2);
        }
        if constexpr (EPI == DG_EPI_ENC || EPI == DG_EPI_GENC) {
            rsum = wave_sum(rsum);
            const int ncb = (p.N + 63) / 64;
            if (lane == 0 && m0 + wm * 64 < p.M && n0 + wn * 64 < p.N) p.rowpart[(int64_t)rblk * ncb + tile_n * 2 + wn] = rsum;
        }
    }
}

template <bool A_KM, bool B_KN, int EPI, bool SPLIT>
int launch_dense_gemm_form(const DenseGemm& p, int splits, hipStream_t stream) {
    static bool attr_done = false;
    if (!attr_done) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&dense_gemm_kernel<A_KM, B_KN, EPI, SPLIT>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, DG_LDS);
        if (e != hipSuccess) {
            pv_set_error(std::string("hipFuncSetAttribute(dense_gemm_kernel): ") + hipGetErrorString(e));
            return PV_ERR_HIP;
        }
        attr_done = true;
    }
    const int ntm = (p.M + DG_BM - 1) / DG_BM, ntn = (p.N + DG_BN - 1) / DG_BN;
    DenseGemm q = p;
    // wide outputs: grouped tile order (the kernel's comment); tuning key dense_group: -1 auto (4 row tiles per group), 0 off, n
    q.group = g_pv_tuning.dense_group >= 0 ? g_pv_tuning.dense_group : (ntn > 16 ? 4 : 0);
    hipLaunchKernelGGL((dense_gemm_kernel<A_KM, B_KN, EPI, SPLIT>), dim3(ntm * ntn, splits), dim3(256), DG_LDS, stream, q);
    PV_LAUNCH_CHECK("dense_gemm_kernel");
    return PV_OK;
}

// ---- operand maxima of the split-fp16 form ---------------------------------------------------------------------------------------
// operand maxima: bit patterns of non-negative floats order like the floats, and a maximum does not depend on the order it is taken in
// the three operands that exist before the first GEMM of a dense step -- sae_in, W_enc^T, W_dec -- in ONE launch (blockIdx.y = tensor):
// slot arrays t * DG_AMAX_SLOTS of `slots`, zeroed at the head of the step (dense_absmax3)
struct AbsmaxArgs { const float* x[3]; int64_t n4[3]; int slot[3]; };
__global__ __launch_bounds__(256) void dense_absmax3_kernel(const AbsmaxArgs a, uint32_t* __restrict__ slots, const uint32_t* __restrict__ gate) {
    if (gate && *gate != 1u) return;
    const int t = blockIdx.y;
    const float* __restrict__ x = a.x[t];
    const int64_t n4 = a.n4[t];
    float m = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0)
        atomicMax(slots + a.slot[t] * DG_AMAX_SLOTS + ((blockIdx.x * 4 + (threadIdx.x >> 6)) & (DG_AMAX_SLOTS - 1)), __float_as_uint(m));
}

// column partials [nblk][d] -> out[j] (+ firing statistics, + per-workgroup totals for l0)
__global__ __launch_bounds__(256) void dense_colreduce_kernel(const float* __restrict__ part, int nblk, int d, float* __restrict__ out,
                                                              float* __restrict__ out2, float* __restrict__ act_freq,
                                                              float* __restrict__ n_since_fired, int update_stats,
                                                              float* __restrict__ block_tot, const uint32_t* __restrict__ gate = nullptr) {
    __shared__ float red[4];
    if (gate && *gate != 1u) return;
    const int j = blockIdx.x * 256 + threadIdx.x;
    float s = 0.f;
    if (j < d) {
#pragma unroll 16
        for (int b = 0; b < nblk; ++b) s += part[(int64_t)b * d + j];        // fixed order; coalesced across the workgroup; 16 loads in flight
                                                                             // (one per trip was 64 dependent round trips: 28 us for 6 MB)
        out[j] = s;
        if (out2) out2[j] = s;
        if (update_stats) {                                                  // train_sae.py:356-361
            act_freq[j] += s;
            n_since_fired[j] = s > 0.f ? 0.f : n_since_fired[j] + 1.f;
        }
    }
    if (block_tot) {
        float t = wave_sum(s);
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        if (lane == 0) red[wv] = t;
        __syncthreads();
        if (threadIdx.x == 0) block_tot[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
    }
}
}  // namespace

template <bool A_KM, bool B_KN, int EPI>
int launch_dense_gemm(const DenseGemm& p, int splits, hipStream_t stream) {
    if constexpr (EPI == DG_EPI_STORE || EPI == DG_EPI_ENC || EPI == DG_EPI_DH || EPI == DG_EPI_GENC || EPI == DG_EPI_ENC_T || EPI == DG_EPI_DH_T) {
        if (p.a_max && p.b_max && !g_pv_tuning.dense_fp32) return launch_dense_gemm_form<A_KM, B_KN, EPI, true>(p, splits, stream);
    }
    return launch_dense_gemm_form<A_KM, B_KN, EPI, false>(p, splits, stream);
}
#define DG_FORM(A_KM, B_KN, EPI) template int launch_dense_gemm<A_KM, B_KN, EPI>(const DenseGemm&, int, hipStream_t)
DG_FORM(false, false, DG_EPI_ENC); DG_FORM(false, false, DG_EPI_ENC_T); DG_FORM(false, false, DG_EPI_DH); DG_FORM(false, false, DG_EPI_DH_T);
DG_FORM(false, false, DG_EPI_GENC); DG_FORM(false, false, DG_EPI_MUL); DG_FORM(false, false, DG_EPI_EXPB); DG_FORM(false, false, DG_EPI_STORE);
DG_FORM(false, true, DG_EPI_STORE); DG_FORM(true, true, DG_EPI_STORE);
#undef DG_FORM

int dense_absmax3(const pv_sae_desc& d, const pv_sae_state* st, const float* sae_in, int N, uint32_t* amax, const uint32_t* gate, hipStream_t stream) {
    const int64_t w4 = (int64_t)d.d_sae * d.d_in / 4;
    const AbsmaxArgs a = {{sae_in, (const float*)st->W_encT, (const float*)st->W_dec}, {(int64_t)N * d.d_in / 4, w4, w4}, {DG_AM_X, DG_AM_WENC, DG_AM_WDEC}};
    PV_HIP_CHECK(hipMemsetAsync(amax, 0, (size_t)PV_SAE_AMAX_TENSORS * DG_AMAX_SLOTS * 4, stream));
    hipLaunchKernelGGL(dense_absmax3_kernel, dim3(1024, 3), dim3(256), 0, stream, a, amax, gate);
    PV_LAUNCH_CHECK("dense_absmax3_kernel");
    return PV_OK;
}

int dense_colreduce(const float* part, int nblk, int d, float* out, float* act_freq, float* n_since_fired, int update_stats, float* blk_tot,
                    const uint32_t* gate, hipStream_t stream) {
    hipLaunchKernelGGL(dense_colreduce_kernel, dim3((d + 255) / 256), dim3(256), 0, stream, part, nblk, d, out, (float*)nullptr, act_freq,
                       n_since_fired, update_stats, blk_tot, gate);
    PV_LAUNCH_CHECK("dense_colreduce_kernel");
    return PV_OK;
}
int dense_colreduce(const float* part, int nblk, int d, float* out, const uint32_t* gate, hipStream_t stream) {
    return dense_colreduce(part, nblk, d, out, nullptr, nullptr, 0, nullptr, gate, stream);
}
