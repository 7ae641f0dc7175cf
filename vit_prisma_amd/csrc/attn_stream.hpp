// The streaming attention body behind attn_stream_kernel<E, DH> (attention.hip: d_head 32 / 64, 640 < T <= PV_ATTN_MAX_TOKENS) and
// attn_wide_kernel<E, DHP> (attention_wide.hip: 64 < d_head <= 128 with d_head % 8 == 0, every T), the launcher of the two, and the
// flop / byte count every attention launcher hands to the profiler.
//
// The shape is attn_lean_kernel's without that kernel's bf16 / d_head 64 specialisations: a WAVE owns 32 query rows of one (image,
// head), the four waves of a workgroup (128 consecutive queries) share each 32-key K / V tile through double-buffered LDS, the keys
// are streamed TWICE with the product swapped (S^T = K Q^T: a lane holds 16 keys of ONE query), so that nothing in LDS or registers
// grows with T:
//   pass 1  per tile: S^T on MFMA (fp32: 32x32x2f32, as attn_kernel<float>; bf16: 32x32x16_bf16), scores = round_T(acc / attn_scale)
//           like the reference's score tensor (the division is the rule -- sqrt(32), sqrt(80), sqrt(88), sqrt(104) are no powers of
//           two; x * (1 / scale) only where the scale is a power of two: d_head 64), online (max, sum) per lane; the two lanes of a
//           query are merged at the end (+ hook_attn_scores, when tapped)
//   pass 2  the same tiles again: p = exp(s - max) / sum, rounded to the storage dtype -> hook_pattern, and z^T += V^T P^T on MFMA.
//           The accumulator tile S^T IS the B operand of that product (its rows = keys are the sum index): register e of a lane is
//           key (e & 3) + 8 (e >> 2) + 4 half, and the V operand is read from LDS in that key order -- fp32: one float per (key, d)
//           of the row-major tile; bf16: two 8-byte reads of the transposed tile V^T [d][32 keys] -- no lane exchange anywhere.
//           z^T leaves the accumulators as 4 consecutive d per register group: 16-byte (fp32) / 8-byte (bf16) stores into the
//           query's own row.
// A row with a NaN / +inf score, or nothing but -inf, becomes zeros (attention.py:148-150), decided per row after pass 1.
// Taps: TW = 2 (fp32) / 4 (bf16) tiles collect in a per-wave LDS window of 32 rows x 256 B and leave as 16-byte stores, 4 rows x 256
// contiguous bytes per instruction, at the row's own alignment (an odd T leaves rows only element-aligned); each element once.
// Whole heads are assigned per XCD (the query blocks of a head share one L2's copy of its K / V).
//
// The body is compiled per padded width DHP.  RAGGED = false (attn_stream_kernel): d_head == DHP, every width below is a constant.
// RAGGED = true (attn_wide_kernel, DHP 96 for d_head 72 - 96, 128 for 104 - 128): the true d_head is a run-time value, and columns
// d_head .. DHP - 1 contribute exact zeros:
//   - Q fragments of 16-byte chunks at or beyond d_head are zero in registers;
//   - the pad columns of both K buffers and both V buffers are written with zeros ONCE before the first tile (uninitialised LDS
//     times a zero Q is NaN when the LDS word happens to be NaN / inf), and staging writes only chunks below d_head;
//   - the fp32 split "half h takes d in [h DHP / 2, (h + 1) DHP / 2)" is the same for Q and K;
//   - z is stored only for d < d_head: d_head % 8 == 0 keeps every 4-wide register group wholly inside or wholly outside.
// CAUSAL = true (attn_causal_kernel, attention_causal.hip: the text tower): the reference's additive mask, -inf where key > query, is
// added to the rounded scores in BOTH passes before anything reads them, so hook_attn_scores holds the masked value, the online max /
// sum see it, and the pattern above the diagonal is exp(-inf) = exactly 0 in the tap and in the P V operand.  Every row keeps its
// diagonal, so a good row's max is finite; tiles wholly above a wave's queries are still multiplied (a NaN there must reach the row).
// The flag is compile-time only: the two non-causal kernels compile to what they compiled to without it.
// LDS: K 2 x 32 x (DHP EB + 16), V the same (bf16: 2 x DHP x 80), windows 32 KiB:
//   <float, 32> 50.0 KiB, <bf16, 32> 42.0 KiB, <bf16, 64> 51.0 KiB = three workgroups per CU, <float, 64> 66.0 KiB = two;
//   <float, 96> 82.0 KiB, <float, 128> 98.0 KiB = one, <bf16, 96> 60.0 KiB, <bf16, 128> 69.0 KiB = two.
// The waves per SIMD each instance is compiled for are the launch bounds of the two kernels; their files state the floors.  The fp32
// instances are bound by the f32 MFMA (1/16 of the bf16 rate: 2 x DHP x 32 cycles per tile and pass), the bf16 ones by VALU issue
// and the tap stream like attn_lean_kernel.
#pragma once
#include "attention.hpp"

#include <cmath>
#include <type_traits>
#include "prof.hpp"

namespace {

// what an attention launch computes and moves: QK^T and PV (2 x 2 B H T^2 d_head flops); q, k, v, z and each tapped [T][T] block once
inline ProfScope attn_prof_scope(const AttnParams& p, int elem_bytes, hipStream_t stream) {
    const double bh = (double)p.B * p.H, tt = (double)p.T * p.T;
    const double bytes = (4.0 * bh * p.T * p.dh + ((p.scores ? 1.0 : 0.0) + (p.pattern ? 1.0 : 0.0)) * bh * tt) * elem_bytes;
    return ProfScope(PV_PROF_ATTN, stream, 4.0 * bh * tt * p.dh, bytes);
}

constexpr int ATTN_VT_ROW = 80;             // V^T tile row (bf16): 32 keys x 2 B + 16 pad

template <typename E, int DHP, bool RAGGED, bool CAUSAL>
__device__ __forceinline__ void attn_stream_body(const AttnParams& p) {
    constexpr int EB = DT<E>::kBytes;
    constexpr bool F32 = EB == 4;
    constexpr int KROW = DHP * EB + 16;                      // bytes per key row of a row-major tile (+16: conflict-free b128 rows)
    constexpr int VBYTES = F32 ? 32 * KROW : DHP * ATTN_VT_ROW;
    constexpr int TW = 8 / EB;                               // tiles per tap window (256-byte rows)
    constexpr int CH = DHP * EB / 16;                        // 16-byte chunks per padded key row
    constexpr int NF = (32 * CH + 255) / 256;                // chunks a thread moves per tile
    constexpr int NTN = DHP / 32;
    constexpr int NQ = F32 ? DHP / 8 : DHP / 16;             // 16-byte Q fragments per lane
    __shared__ __attribute__((aligned(16))) unsigned char Kst[2][32 * KROW];
    __shared__ __attribute__((aligned(16))) unsigned char Vst[2][VBYTES];
    __shared__ __attribute__((aligned(16))) unsigned char win[4][32 * 256];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int T_ = p.T, H = p.H, dh = RAGGED ? p.dh : DHP;
    const int chr = dh * EB / 16;                            // 16-byte chunks of a true key row (d_head % 8 == 0)
    const int qblocks = (T_ + 127) / 128;
    int bid = blockIdx.x;                                    // whole heads per XCD, as in attn_lean_kernel
    {
        const int heads = p.B * H, per_xcd = heads / 8;
        if (bid < per_xcd * 8 * qblocks) {
            const int xcd = bid & 7, i = bid >> 3;
            bid = ((i / qblocks) * 8 + xcd) * qblocks + i % qblocks;
        }
    }
    const int g = bid / qblocks;                             // (image, head)
    const int q0 = (bid - g * qblocks) * 128 + wave * 32;
    const bool active = q0 < T_;                             // idle waves of a head's last block still stage tiles and meet the barriers
    const int b = g / H, h = g - b * H;
    const int half = lane >> 5, l31 = lane & 31;
    unsigned char* L = win[wave];
    const int64_t tokb = (int64_t)H * dh * EB;               // bytes between tokens of one head
    const int64_t head_off = (((int64_t)b * T_ * H + h) * dh) * EB;
    const unsigned char* qg = reinterpret_cast<const unsigned char*>(p.q) + head_off;
    const unsigned char* kg = reinterpret_cast<const unsigned char*>(p.k) + head_off;
    const unsigned char* vg = reinterpret_cast<const unsigned char*>(p.v) + head_off;
    const int ntile = (T_ + 31) / 32;

    if constexpr (RAGGED) {
        // the pad columns of every K / V buffer: zeros, once (nothing below writes them again).  Row-major tiles: chunks chr .. CH - 1
        // of each of the 32 key rows; the bf16 V^T tile: its rows d >= d_head, whole
        for (int idx = tid; idx < 32 * CH; idx += 256) {
            const int key = idx & 31, ch = idx >> 5;
            if (ch >= chr) {
                *reinterpret_cast<uint4*>(Kst[0] + key * KROW + ch * 16) = make_uint4(0, 0, 0, 0);
                *reinterpret_cast<uint4*>(Kst[1] + key * KROW + ch * 16) = make_uint4(0, 0, 0, 0);
                if constexpr (F32) {
                    *reinterpret_cast<uint4*>(Vst[0] + key * KROW + ch * 16) = make_uint4(0, 0, 0, 0);
                    *reinterpret_cast<uint4*>(Vst[1] + key * KROW + ch * 16) = make_uint4(0, 0, 0, 0);
                }
            }
        }
        if constexpr (!F32) {
            for (int idx = tid; idx < DHP * (ATTN_VT_ROW / 16); idx += 256) {
                if (idx / (ATTN_VT_ROW / 16) >= dh) {
                    *reinterpret_cast<uint4*>(Vst[0] + idx * 16) = make_uint4(0, 0, 0, 0);
                    *reinterpret_cast<uint4*>(Vst[1] + idx * 16) = make_uint4(0, 0, 0, 0);
                }
            }
        }
    }

    // Q as the B operand (columns = this wave's queries).  bf16: lane (query l31, half) holds d-chunk 2 c + half; fp32: the f32
    // MFMA sums two d per step, one per half -- the order of the sum is free, so half h takes d in [h DHP / 2, (h + 1) DHP / 2)
    // (contiguous 16-byte loads) and so do the K fragments.  Chunks at or beyond d_head: zeros
    uint4 qf[NQ];
    {
        const int qi = q0 + l31;
#pragma unroll
        for (int c = 0; c < NQ; ++c) {
            const int ch = F32 ? half * (DHP / 8) + c : 2 * c + half;
            qf[c] = (qi < T_ && ch < chr) ? *reinterpret_cast<const uint4*>(qg + qi * tokb + ch * 16) : make_uint4(0, 0, 0, 0);
        }
    }

    // cooperative tile fetch: chunk idx = tid + 256 i -> 16 B (chunk idx / 32) of key row idx % 32; rows >= T read 0 (K: masked
    // scores; V: 0 x 0, never 0 x garbage); chunks at or beyond d_head are neither read nor parked
    auto fetch = [&](const unsigned char* base, int kt, uint4 (&r)[NF]) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            const int idx = tid + 256 * i, key = kt * 32 + (idx & 31), ch = idx >> 5;
            r[i] = (ch < chr && key < T_) ? *reinterpret_cast<const uint4*>(base + key * tokb + ch * 16) : make_uint4(0, 0, 0, 0);
        }
    };
    auto park_rows = [&](unsigned char* dst, const uint4 (&r)[NF]) __attribute__((always_inline)) {         // row-major [32 keys][KROW]
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            const int idx = tid + 256 * i, key = idx & 31, ch = idx >> 5;
            if (ch < chr) *reinterpret_cast<uint4*>(dst + key * KROW + ch * 16) = r[i];
        }
    };
    auto park_v = [&](unsigned char* dst, const uint4 (&r)[NF]) __attribute__((always_inline)) {
        if constexpr (F32) {
            park_rows(dst, r);
        } else {                                                             // 8 d-values of one key -> V^T[d][key] (attn_lean_kernel's stage_v)
#pragma unroll
            for (int i = 0; i < NF; ++i) {
                const int idx = tid + 256 * i, key = idx & 31, ch = idx >> 5;
                if (ch < chr) {
                    const uint32_t w[4] = {r[i].x, r[i].y, r[i].z, r[i].w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        *reinterpret_cast<unsigned short*>(dst + (ch * 8 + 2 * j) * ATTN_VT_ROW + key * 2) = (unsigned short)(w[j] & 0xffffu);
                        *reinterpret_cast<unsigned short*>(dst + (ch * 8 + 2 * j + 1) * ATTN_VT_ROW + key * 2) = (unsigned short)(w[j] >> 16);
                    }
                }
            }
        }
    };

    // S^T tile out of a K tile: sc[e] = the score of key kt * 32 + (e & 3) + 8 (e >> 2) + 4 half against query q0 + l31, scaled and
    // rounded to the storage dtype (x * (1 / scale) is x / scale exactly when the scale is a power of two; otherwise divide)
    const float inv_scale = 1.0f / p.attn_scale;
    const bool scale_pow2 = (__float_as_uint(p.attn_scale) & 0x007fffffu) == 0u && p.attn_scale > 0.f;
    auto score_tile = [&](const unsigned char* kb, float (&sc)[16]) __attribute__((always_inline)) {
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
        for (int c = 0; c < NQ; ++c) {
            if constexpr (F32) {
                const uint4 kf = *reinterpret_cast<const uint4*>(kb + l31 * KROW + (half * (DHP / 2) + 4 * c) * 4);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(kf.x), __uint_as_float(qf[c].x), acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(kf.y), __uint_as_float(qf[c].y), acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(kf.z), __uint_as_float(qf[c].z), acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(kf.w), __uint_as_float(qf[c].w), acc, 0, 0, 0);
            } else {
                const uint4 kf = *reinterpret_cast<const uint4*>(kb + l31 * KROW + (2 * c + half) * 16);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, kf), __builtin_bit_cast(bf16x8, qf[c]), acc, 0, 0, 0);
            }
        }
        if (scale_pow2) {
#pragma unroll
            for (int e = 0; e < 16; ++e) sc[e] = DT<E>::round(acc[e] * inv_scale);
        } else {
#pragma unroll
            for (int e = 0; e < 16; ++e) sc[e] = DT<E>::round(acc[e] / p.attn_scale);
        }
    };

    // Taps: a lane's four groups of 4 consecutive keys go into the wave's LDS window [32 rows][TW tiles x 32 keys] (16-byte chunk c
    // of row r at position c ^ (r & 15)); every TW-th tile (and after the last) the window leaves as 16-byte stores
    auto tap_put = [&](int kt, const float (&v)[16]) __attribute__((always_inline)) {
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            if constexpr (F32) {
                const int c = (kt & (TW - 1)) * 8 + 2 * g4 + half;
                *reinterpret_cast<float4*>(L + l31 * 256 + ((c ^ (l31 & 15)) * 16)) = make_float4(v[4 * g4], v[4 * g4 + 1], v[4 * g4 + 2], v[4 * g4 + 3]);
            } else {
                const int c = (kt & (TW - 1)) * 4 + g4;
                *reinterpret_cast<uint2*>(L + l31 * 256 + ((c ^ (l31 & 15)) * 16) + 8 * half) =
                    make_uint2(pack_bf16x2(v[4 * g4], v[4 * g4 + 1]), pack_bf16x2(v[4 * g4 + 2], v[4 * g4 + 3]));
            }
        }
    };
    const int st_row = lane >> 4, st_ch = lane & 15;
    auto tap_flush = [&](unsigned char* dst, int kt) __attribute__((always_inline)) {
        if ((kt & (TW - 1)) != TW - 1 && kt + 1 < ntile) return;
        __builtin_amdgcn_wave_barrier();
        const int k0 = (kt & ~(TW - 1)) * 32;                                // first key of the window
        const int nb = min(256, (T_ - k0) * EB);                             // valid bytes per row
#pragma unroll 2
        for (int it = 0; it < 8; ++it) {
            const int row = st_row + 4 * it;
            if (q0 + row < T_ && st_ch * 16 < nb) {
                const unsigned char* src = L + row * 256 + ((st_ch ^ (row & 15)) * 16);
                unsigned char* d = dst + ((int64_t)(q0 + row) * T_ + k0) * EB + st_ch * 16;
                if (st_ch * 16 + 16 <= nb) {
                    const uint4 r = *reinterpret_cast<const uint4*>(src);
                    using V = std::conditional_t<F32, pv_u32x4_a4, pv_u32x4_a2>;
                    pv_store16_as<PV_ST_PLAIN, V>(d, r.x, r.y, r.z, r.w);
                } else {
                    for (int e = 0; e < (nb - st_ch * 16) / EB; ++e)
                        reinterpret_cast<E*>(d)[e] = reinterpret_cast<const E*>(src)[e];
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    };
    auto key_masked = [&](int kt, int e) __attribute__((always_inline)) { return kt * 32 + (e & 3) + 8 * (e >> 2) + 4 * half >= T_; };
    // CAUSAL: the reference ADDS its mask to the rounded scores (attention.py:262-265 with base_text_transformer.py:188-194: -inf
    // where key > query, 0 elsewhere).  The add is kept an add: a masked NaN / +inf score becomes NaN, which zeroes its row below
    auto add_causal_mask = [&](int kt, float (&sc)[16]) __attribute__((always_inline)) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int key = kt * 32 + (e & 3) + 8 * (e >> 2) + 4 * half;
            sc[e] = sc[e] + (key > q0 + l31 ? -INFINITY : 0.f);
        }
    };

    // ---- pass 1: online max / sum (and the score tap)
    unsigned char* sc_dst = p.scores ? reinterpret_cast<unsigned char*>(p.scores) + (int64_t)g * T_ * T_ * EB : nullptr;
    float m = -INFINITY, l = 0.f;
    auto pass1_tile = [&](int kt) __attribute__((always_inline)) {
        float sc[16];
        score_tile(Kst[kt & 1], sc);
        if constexpr (CAUSAL) add_causal_mask(kt, sc);
        if (sc_dst) tap_put(kt, sc);
        if (kt + 1 == ntile) {
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (key_masked(kt, e)) sc[e] = -INFINITY;
        }
        float tm = sc[0];
#pragma unroll
        for (int e = 1; e < 16; ++e) tm = fmaxf(tm, sc[e]);
        const float mn = fmaxf(m, tm);
        const float mb = mn == -INFINITY ? 0.f : mn;                          // nothing but -inf so far: exp(-inf - 0) = 0, not exp(NaN)
        float sum = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) sum += __expf(sc[e] - mb);
        l = l * __expf(m - mb) + sum;
        m = mn;
    };
    uint4 kn1[NF], kn2[NF];
    fetch(kg, 0, kn2);
    fetch(kg, 1, kn1);
    park_rows(Kst[0], kn2);
    // per tile, as in attn_lean_kernel: issue the fetch of tile kt + 2 -> multiply tile kt out of LDS -> park tile kt + 1 in the other
    // buffer (free since the barrier that ended tile kt - 1) -> flush the tap window when it is due -> barrier.  (This first barrier
    // also publishes the zeroed pad columns.)
    __syncthreads();
    for (int kt = 0; kt < ntile; ++kt) {
        fetch(kg, kt + 2, kn2);
        if (active) pass1_tile(kt);
        park_rows(Kst[(kt + 1) & 1], kn1);
        if (active && sc_dst) tap_flush(sc_dst, kt);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NF; ++i) kn1[i] = kn2[i];
    }
    {   // merge the two lanes of a query
        const float mo = __shfl_xor(m, 32, 64), lo = __shfl_xor(l, 32, 64);
        const float M = fmaxf(m, mo);
        const float Mb = M == -INFINITY ? 0.f : M;
        l = l * __expf(m - Mb) + lo * __expf(mo - Mb);
        m = M;
    }
    // a row with an infinite / NaN score (or none at all) is NaN throughout in the reference -> zeros (attention.py:149)
    const bool row_ok = l > 0.f && l < INFINITY && m > -INFINITY && m < INFINITY;
    const float inv_l = row_ok ? 1.0f / l : 0.f;
    const float mrow = row_ok ? m : 0.f;

    // ---- pass 2: pattern tap + z
    unsigned char* pt_dst = p.pattern ? reinterpret_cast<unsigned char*>(p.pattern) + (int64_t)g * T_ * T_ * EB : nullptr;
    f32x16 zacc[NTN];
#pragma unroll
    for (int tn = 0; tn < NTN; ++tn)
#pragma unroll
        for (int e = 0; e < 16; ++e) zacc[tn][e] = 0.f;
    auto pass2_tile = [&](int kt) __attribute__((always_inline)) {
        float pr[16];
        score_tile(Kst[kt & 1], pr);
        if constexpr (CAUSAL) add_causal_mask(kt, pr);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float x = DT<E>::round(__expf(pr[e] - mrow) * inv_l);       // attention.py:152 pattern.to(cfg.dtype)
            pr[e] = row_ok ? x : 0.f;
        }
        if (kt + 1 == ntile) {
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (key_masked(kt, e)) pr[e] = 0.f;
        }
        if (pt_dst) tap_put(kt, pr);
        const unsigned char* vb = Vst[kt & 1];
        if constexpr (F32) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int key = (e & 3) + 8 * (e >> 2) + 4 * half;
#pragma unroll
                for (int tn = 0; tn < NTN; ++tn) {
                    const float vv = *reinterpret_cast<const float*>(vb + key * KROW + (tn * 32 + l31) * 4);
                    zacc[tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(vv, pr[e], zacc[tn], 0, 0, 0);
                }
            }
        } else {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                // element j of this lane's fragment = register 8 s + j = key 16 s + 8 (j >> 2) + 4 half + (j & 3)
                const pv_u32x4_a16 pb = {pack_bf16x2(pr[8 * s], pr[8 * s + 1]), pack_bf16x2(pr[8 * s + 2], pr[8 * s + 3]),
                                         pack_bf16x2(pr[8 * s + 4], pr[8 * s + 5]), pack_bf16x2(pr[8 * s + 6], pr[8 * s + 7])};
#pragma unroll
                for (int tn = 0; tn < NTN; ++tn) {
                    const unsigned char* vr = vb + (tn * 32 + l31) * ATTN_VT_ROW + (16 * s + 4 * half) * 2;
                    const uint2 lo = *reinterpret_cast<const uint2*>(vr), hi = *reinterpret_cast<const uint2*>(vr + 16);
                    const pv_u32x4_a16 va = {lo.x, lo.y, hi.x, hi.y};
                    zacc[tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, va), __builtin_bit_cast(bf16x8, pb), zacc[tn], 0, 0, 0);
                }
            }
        }
    };
    uint4 vn1[NF], vn2[NF];
    fetch(kg, 0, kn2);
    fetch(vg, 0, vn2);
    fetch(kg, 1, kn1);
    fetch(vg, 1, vn1);
    park_rows(Kst[0], kn2);        // (everyone left pass 1's last tile through its closing barrier)
    park_v(Vst[0], vn2);
    __syncthreads();
    for (int kt = 0; kt < ntile; ++kt) {
        fetch(kg, kt + 2, kn2);
        fetch(vg, kt + 2, vn2);
        if (active) pass2_tile(kt);
        park_rows(Kst[(kt + 1) & 1], kn1);
        park_v(Vst[(kt + 1) & 1], vn1);
        if (active && pt_dst) tap_flush(pt_dst, kt);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            kn1[i] = kn2[i];
            vn1[i] = vn2[i];
        }
    }
    if (!active) return;

    // ---- z [B, T, H, dh]: zacc[tn][e] = z[query q0 + l31][d = 32 tn + (e & 3) + 8 (e >> 2) + 4 half], stored for d < d_head
    const int qi = q0 + l31;
    if (qi < T_) {
        unsigned char* zr = reinterpret_cast<unsigned char*>(p.z) + head_off + qi * tokb;
#pragma unroll
        for (int tn = 0; tn < NTN; ++tn)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int d0 = 32 * tn + 8 * g4 + 4 * half;
                if (d0 < dh) {
                    const float a0 = zacc[tn][4 * g4], a1 = zacc[tn][4 * g4 + 1], a2 = zacc[tn][4 * g4 + 2], a3 = zacc[tn][4 * g4 + 3];
                    if constexpr (F32) *reinterpret_cast<float4*>(zr + d0 * 4) = make_float4(a0, a1, a2, a3);
                    else *reinterpret_cast<uint2*>(zr + d0 * 2) = make_uint2(pack_bf16x2(a0, a1), pack_bf16x2(a2, a3));
                }
            }
    }
}

// one launch of either kernel: a workgroup per 128 queries of one (image, head)
template <typename E>
int launch_attn_streaming(void (*kernel)(const AttnParams), const char* name, const AttnParams& p, hipStream_t stream) {
    constexpr int EB = DT<E>::kBytes;
    const int64_t blocks = (int64_t)p.B * p.H * ((p.T + 127) / 128);
    PV_REQUIRE(blocks < (1ll << 31), "attention grid");
    PV_REQUIRE((int64_t)p.T * p.H * p.dh * EB < (1ll << 31), "attention: T * H * d_head bytes per image must stay below 2^31");
    PV_REQUIRE(pv_aligned16(p.z), "attention output must be 16-byte aligned");
    {
        ProfScope prof = attn_prof_scope(p, EB, stream);
        hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, stream, p);
    }
    PV_LAUNCH_CHECK(name);
    return PV_OK;
}

}  // namespace
