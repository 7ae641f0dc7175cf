// What more than one GEMM kernel file uses (gemm_generic.hip, gemm_v4.hpp, gemm_tiled.hpp; index in gemm.hip): the debug trace's
// stamp, the bf16 pack / unpack and the activations, the run-time and the compile-time store epilogues of an 8-element chunk, the
// staging geometry of the two MFMA shapes, and the profiler's cost of a launch.  Everything is inlined where it is used.
// (Ordinary inline functions at global scope, as the helpers of pv_common.hpp.)
#pragma once
#include "gemm_impl.hpp"

#include "kloop.hpp"
#include "prof.hpp"

// debug tracing (pv_debug_gemm_trace_*): stamps on the 100 MHz wall clock, written by thread 0 of each workgroup
__device__ __forceinline__ void trace_stamp(uint64_t* trace, int bid, int slot) {
    if (trace && threadIdx.x == 0) {
        trace[(int64_t)bid * 4 + slot] = wall_clock64();
        if (slot == 0) trace[(int64_t)bid * 4 + 3] = ((uint64_t)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32) |
                                                      (uint64_t)__builtin_amdgcn_s_getreg((31 << 11) | 4);
    }
}

__device__ __forceinline__ pv_f32x2 unpack2(uint32_t w) {
    return pv_f32x2{__uint_as_float(w << 16), __uint_as_float(w & 0xffff0000u)};
}
__device__ __forceinline__ uint32_t pack2(pv_f32x2 v) { return pack_bf16x2(v.x, v.y); }

template <int ACT>
__device__ __forceinline__ pv_f32x2 act2(pv_f32x2 x) {
    if constexpr (ACT == PV_ACT_QUICK_GELU) {                // x * sigmoid(1.702 x), models/activation_fns.py:19
        const pv_f32x2 t = x * (-1.702f * 1.4426950408889634f);
        pv_f32x2 d = {__builtin_amdgcn_exp2f(t.x), __builtin_amdgcn_exp2f(t.y)};
        d = d + 1.0f;
        const pv_f32x2 r = {__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
        return x * r;
    } else if constexpr (ACT == PV_ACT_GELU) {               // 0.5 x (1 + erf(x / sqrt 2)); erf: Abramowitz-Stegun 7.1.26
        const pv_f32x2 z = x * 0.70710678118654752440f;
        const pv_f32x2 az = __builtin_elementwise_abs(z);
        const pv_f32x2 den = __builtin_elementwise_fma(az, pv_f32x2{0.3275911f, 0.3275911f}, pv_f32x2{1.0f, 1.0f});
        const pv_f32x2 t = {__builtin_amdgcn_rcpf(den.x), __builtin_amdgcn_rcpf(den.y)};
        pv_f32x2 q = __builtin_elementwise_fma(t, pv_f32x2{1.061405429f, 1.061405429f}, pv_f32x2{-1.453152027f, -1.453152027f});
        q = __builtin_elementwise_fma(t, q, pv_f32x2{1.421413741f, 1.421413741f});
        q = __builtin_elementwise_fma(t, q, pv_f32x2{-0.284496736f, -0.284496736f});
        q = __builtin_elementwise_fma(t, q, pv_f32x2{0.254829592f, 0.254829592f});
        q = q * t;
        const pv_f32x2 a2 = az * az * (-1.4426950408889634f);
        const pv_f32x2 e = {__builtin_amdgcn_exp2f(a2.x), __builtin_amdgcn_exp2f(a2.y)};
        pv_f32x2 r = __builtin_elementwise_fma(-q, e, pv_f32x2{1.0f, 1.0f});
        r = __builtin_elementwise_copysign(r, z);
        const pv_f32x2 hx = x * 0.5f;
        return __builtin_elementwise_fma(hx, r, hx);
    } else {
        // F.relu keeps a NaN; v_max_f32 / v_pk_max_f32 (maxnum) would return the 0 beside it.  A compare that NaN fails selects x.
        return pv_f32x2{x.x < 0.0f ? 0.0f : x.x, x.y < 0.0f ? 0.0f : x.y};
    }
}

// The activation every bf16 epilogue applies (v4's run-time epilogues included): ONE instruction sequence for all
// kernels, so mlp.hook_post of an image has the same bits whatever GEMM kernel its batch size selects.
template <typename T>
__device__ __forceinline__ float act_any(float x, int act) {
    if constexpr (sizeof(T) == 2) {
        const pv_f32x2 v = {x, x};
        if (act == PV_ACT_GELU) return act2<PV_ACT_GELU>(v).x;
        if (act == PV_ACT_QUICK_GELU) return act2<PV_ACT_QUICK_GELU>(v).x;
        return act2<PV_ACT_RELU>(v).x;
    } else {
        return pv_act<false>(x, act);
    }
}

// (store policy, pv_common.hpp: the run-time epilogues put every 16-byte store in the CONSUMED class, their tap outputs included --
// they have always been plain stores here, and these kernels are not on the bf16 forwards' hot path; the ragged tail stays scalar)
template <typename T>
__device__ __forceinline__ void epilogue8(const GemmParams& p, float (&v)[8], int gm, int gn) {
    T* out0 = reinterpret_cast<T*>(p.out0);
    T* out1 = reinterpret_cast<T*>(p.out1);
    const T* bias = reinterpret_cast<const T*>(p.bias0);
    int col = gn;
    if (p.epi == PV_EPI_QKV) {
        const int which = gn / p.nsplit;
        col = gn - which * p.nsplit;
        if (which == 1) { out0 = reinterpret_cast<T*>(p.out1); bias = reinterpret_cast<const T*>(p.bias1); }
        if (which == 2) { out0 = reinterpret_cast<T*>(p.out2); bias = reinterpret_cast<const T*>(p.bias2); }
    }
    const int nvalid = min(8, p.N - gn);
    if (p.vec_out && nvalid == 8) {
        if (bias) {
            float b[8];
            load8(bias + col, b);
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] += b[i];
        }
        if (p.epi == PV_EPI_BIAS || p.epi == PV_EPI_QKV) {
            store8_consumed(out0 + (int64_t)gm * p.ldo + col, v);
        } else if (p.epi == PV_EPI_RESID) {
            // attn_out / mlp_out is rounded to the storage dtype first (it is what the reference
            // adds to the residual: transformer_block.py:122-124, :134)
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = DT<T>::round(v[i]);
            if (out0) store8_consumed(out0 + (int64_t)gm * p.ldo + gn, v);
            float r[8];
            load8(reinterpret_cast<const T*>(p.resid) + (int64_t)gm * p.ldr + gn, r);
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] += r[i];
            store8_consumed(out1 + (int64_t)gm * p.ldo + gn, v);
        } else {  // PV_EPI_ACT: mlp.py:67-72, activation applied to the stored pre-activation
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = DT<T>::round(v[i]);
            if (out0) store8_consumed(out0 + (int64_t)gm * p.ldo + gn, v);
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = act_any<T>(v[i], p.act);
            store8_consumed(out1 + (int64_t)gm * p.ldo + gn, v);
        }
    } else {
        for (int i = 0; i < nvalid; ++i) {
            float x = v[i];
            int c = col + i, g = gn + i;
            T* o0 = out0;
            const T* bs = bias;
            if (p.epi == PV_EPI_QKV) {   // a chunk may straddle outputs when nsplit % 8 != 0
                const int which = g / p.nsplit;
                c = g - which * p.nsplit;
                o0 = reinterpret_cast<T*>(which == 0 ? p.out0 : (which == 1 ? p.out1 : p.out2));
                bs = reinterpret_cast<const T*>(which == 0 ? p.bias0 : (which == 1 ? p.bias1 : p.bias2));
            }
            if (bs) x += DT<T>::load(bs + c);
            if (p.epi == PV_EPI_BIAS || p.epi == PV_EPI_QKV) {
                DT<T>::store(o0 + (int64_t)gm * p.ldo + c, x);
            } else if (p.epi == PV_EPI_RESID) {
                x = DT<T>::round(x);
                if (o0) DT<T>::store(o0 + (int64_t)gm * p.ldo + g, x);
                x += DT<T>::load(reinterpret_cast<const T*>(p.resid) + (int64_t)gm * p.ldr + g);
                DT<T>::store(out1 + (int64_t)gm * p.ldo + g, x);
            } else {
                x = DT<T>::round(x);
                if (o0) DT<T>::store(o0 + (int64_t)gm * p.ldo + g, x);
                DT<T>::store(out1 + (int64_t)gm * p.ldo + g, act_any<T>(x, p.act));
            }
        }
    }
}

// epilogue8 with the bias values and the residual chunk already in registers (bf16 storage; the full-chunk
// vector case only).  Same arithmetic, same rounding points as epilogue8.
template <typename T>
__device__ __forceinline__ void epilogue8_pre(const GemmParams& p, float (&v)[8], int gm, int gn, int col, T* out0,
                                              const uint4& braw, const uint4& res) {
    T* out1 = reinterpret_cast<T*>(p.out1);
    const uint32_t bw[4] = {braw.x, braw.y, braw.z, braw.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[2 * i] += __uint_as_float(bw[i] << 16);
        v[2 * i + 1] += __uint_as_float(bw[i] & 0xffff0000u);
    }
    if (p.epi == PV_EPI_BIAS || p.epi == PV_EPI_QKV) {
        store8_consumed(out0 + (int64_t)gm * p.ldo + col, v);
    } else if (p.epi == PV_EPI_RESID) {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = DT<T>::round(v[i]);
        if (out0) store8_consumed(out0 + (int64_t)gm * p.ldo + gn, v);
        const uint32_t rw[4] = {res.x, res.y, res.z, res.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[2 * i] += __uint_as_float(rw[i] << 16);
            v[2 * i + 1] += __uint_as_float(rw[i] & 0xffff0000u);
        }
        store8_consumed(out1 + (int64_t)gm * p.ldo + gn, v);
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = DT<T>::round(v[i]);
        if (out0) store8_consumed(out0 + (int64_t)gm * p.ldo + gn, v);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = act_any<T>(v[i], p.act);
        store8_consumed(out1 + (int64_t)gm * p.ldo + gn, v);
    }
}

// what the profiler books for a launch: its flops and its algorithmic bytes (each operand once, the outputs of its epilogue)
struct GemmCost { double flops, bytes; };
template <typename T>
GemmCost gemm_cost(const GemmParams& p) {
    const double mn = (double)p.M * p.N;
    double outs = 1.0;                                              // BIAS / QKV: one M x N store
    if (p.epi == PV_EPI_RESID) outs = 2.0 + (p.out0 ? 1.0 : 0.0);   // resid read + out1 (+ tap)
    if (p.epi == PV_EPI_ACT) outs = 1.0 + (p.out0 ? 1.0 : 0.0);
    return {2.0 * mn * p.K, ((double)p.M * p.K + (double)p.N * p.K + outs * mn) * DT<T>::kBytes};
}

// The MFMA shape of the bf16 kernels v4 / v7 / v8 (kloop.hpp: 16x16x32 unless built with -DPV_GEMM_MFMA=32) and what it does to
// their store epilogues.  These transpose a 32-row block of the wave's accumulators through LDS in four PASSES of 8 rows x 64
// columns; in a pass lane l stores the 8-column chunk l & 7 of the pass's row l >> 3.  With 32x32x16 accumulators a pass is 8
// consecutive rows.  With 16x16x32 ones (row = 4 * (lane >> 4) + reg inside a 16-row block) a pass takes register pair
// 2 * (it & 1) of block it >> 1 from every lane, so that all 64 lanes stage 8 values per pass as before: its rows are
// 16 * (it >> 1) + 2 * (it & 1) + {0, 1, 4, 5, 8, 9, 12, 13}.  The four lane groups of a staged row pair would hit the same banks
// (rows are 256 bytes): the 16-column block nj of a row staged by lane group g sits at position nj ^ g.
constexpr bool S16 = kloop::Shape<kloop::Bf16>::S16;
template <bool S> __device__ __forceinline__ constexpr int epi_pass_row(int it) { return S ? (it >> 1) * 16 + (it & 1) * 2 : it * 8; }
template <bool S> __device__ __forceinline__ int epi_lane_row(int lane) {
    const int j8 = lane >> 3;
    return S ? 4 * (j8 >> 1) + (j8 & 1) : j8;
}
// where (in floats) lane l reads its chunk of a pass's 8 x 64 staging rows
template <bool S> __device__ __forceinline__ int epi_read_off(int lane) {
    const int j8 = lane >> 3, c8 = lane & 7;
    return S ? j8 * 64 + (((c8 >> 1) ^ (j8 >> 1)) * 16 + (c8 & 1) * 8) : j8 * 64 + c8 * 8;
}
// 16x16x32: pass it of a 32-row block (its two accumulators; kloop.hpp for the quarters) -> the 8 x 64 floats at Cp
__device__ __forceinline__ void stage_pass16(float* Cp, const f32x16 (&blk)[2], int it, int lane) {
    const int g = lane >> 4, l15 = lane & 15;
#pragma unroll
    for (int nj = 0; nj < 4; ++nj)
#pragma unroll
        for (int rr = 0; rr < 2; ++rr)
            Cp[(2 * g + rr) * 64 + ((nj ^ g) * 16 + l15)] = blk[nj >> 1][4 * (2 * (it >> 1) + (nj & 1)) + 2 * (it & 1) + rr];
}

// ---------------------------------------------------------------------------------------------------
// bf16 store epilogue with everything known at compile time (v7).  The phase trace (tools/gemm_trace.py)
// showed the generic epilogue8 to be VALU-bound, not store-bound: the MLP-1 tile spent 35 us in it against
// 28 us in its K loop (IEEE division + three activation arms + per-call pointer math, ~100 VALU per element
// for 8 waves per CU).  Here: packed fp32 math (v_pk_*), v_exp / v_rcp instead of expf / division (the value
// is rounded to bf16 two instructions later), no run-time switches.
// ---------------------------------------------------------------------------------------------------
// one 8-element chunk: acc + bias -> (rounded) outputs.  o0 / o1 point at the chunk; b = unpacked bias.
template <int EPI, int ACT>
__device__ __forceinline__ void epi8_bf16(const float4& x0, const float4& x1, const pv_f32x2 (&b)[4], bf16_t* o0, bf16_t* o1,
                                          const uint4& res) {
    pv_f32x2 v[4] = {{x0.x, x0.y}, {x0.z, x0.w}, {x1.x, x1.y}, {x1.z, x1.w}};
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = v[i] + b[i];
    uint4 r;
    r.x = pack2(v[0]); r.y = pack2(v[1]); r.z = pack2(v[2]); r.w = pack2(v[3]);
    if constexpr (EPI == PV_EPI_BIAS || EPI == PV_EPI_QKV) {
        pv_store16_consumed<pv_u32x4_a16>(o0, r.x, r.y, r.z, r.w);
    } else {
        // the stored (bf16-rounded) value is what the reference carries on: transformer_block.py:122-124, :134;
        // mlp.py:67-72
        if (o0) pv_store16_stream<pv_u32x4_a16>(o0, r.x, r.y, r.z, r.w);     // (o0 = the tap-only output of these two epilogues)
        const uint32_t rw[4] = {r.x, r.y, r.z, r.w};
        uint4 y;
        if constexpr (EPI == PV_EPI_RESID) {
            const uint32_t sw[4] = {res.x, res.y, res.z, res.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = unpack2(rw[i]) + unpack2(sw[i]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = act2<ACT>(unpack2(rw[i]));
        }
        y.x = pack2(v[0]); y.y = pack2(v[1]); y.z = pack2(v[2]); y.w = pack2(v[3]);
        pv_store16_consumed<pv_u32x4_a16>(o1, y.x, y.y, y.z, y.w);
    }
}
