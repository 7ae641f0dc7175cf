// The GEMMs of the ViT forward for gfx950, fp32 and bf16, with fused tap epilogues (bias / QKV split / residual add / activation;
// "fused hook-tap": caching an activation costs one HBM store from the epilogue, nothing is re-read).  All of them compute
// C[M][N] = A[M][K] . Bt[N][K]^T.  This file decides: choose() picks, for one launch, among four kernel generations, and
// pv_launch_gemm() launches what it picked and describes exactly that to the debug trace.  The kernels live in files of their own;
// two translation units compile them: gemm_generic.hip, and this one, which includes gemm_v4.hpp and gemm_tiled.hpp below.
//   gemm_generic.hip  gemm_kernel      128 x 128 tile, 256 threads, operands staged through registers into padded LDS rows,
//                                      double-buffered.  Both dtypes, any alignment, patch gather, [K][N] B operand: the kernel for
//                                      whatever the others do not take.  Also act_rows_kernel / pv_launch_act.
//   gemm_v4.hpp       gemm_kernel_v4   128 x 128 tile, operands DMA'd straight into a three-slot LDS ring, three workgroups per CU.
//                                      (Why it shares a translation unit with the tiled family: the head of gemm_v4.hpp.)
//   gemm_tiled.hpp    gemm_kernel_v7   bf16, ONE 512-thread workgroup per CU, (64*MB) x 256 tile, template parameter LP = K-loop
//                                      form: 0 barrier-then-fetch (patch gather, K tails), 1 software-pipelined 64-byte slabs,
//                                      2 full-line 128-byte slabs (with the residual park, -DPV_GEMM_RESID_PARK).
//                     gemm_kernel_v8   v7's full-line form made persistent: a workgroup walks its tiles, their K slabs one stream.
//   gemm_epi.hpp      what more than one of these files uses: the trace stamp, the activation and epilogue helpers, the staging
//                     geometry of the two MFMA shapes, the profiler's cost of a launch.
//   gemm_impl.hpp     GemmChoice and the three launchers: what crosses the translation units.
// bf16 in v4 / v7 / v8 multiplies on v_mfma_f32_16x16x32_bf16 (the higher clock under the power cap, DESIGN.md 3.6;
// -DPV_GEMM_MFMA=32: the 32x32x16 shape in all three, for A/B builds); every one of them accumulates an output in 32-element groups
// of k in rising order, so results do not depend on the kernel picked.  gemm_kernel stays on 32x32x16 (it serves only shapes the
// others cannot take).
// The K loops of v7 and v8 -- slot geometry, swizzles, step bodies, drivers -- and the XCD-aware tile order live in kloop.hpp,
// shared with the SAE filter GEMM (sae_enc_gemm.hip); the kernels keep their LDS objects, descriptors, piece sources and epilogues.
#include <atomic>

#include "gemm_impl.hpp"

#include "prof.hpp"

// the kernels and launchers this translation unit compiles
#include "gemm_v4.hpp"
#include "gemm_tiled.hpp"

namespace {

// CUs a launch may count on: the launch's own budget (a plan's pipeline on CU-masked streams), else the tuning override, else the
// current device's count (cached per device id; rounded down to a multiple of the XCD count: bid and bid + grid on one XCD)
inline int pv_gemm_cus(const GemmParams& p) {
    int n = p.cus > 0 ? p.cus : g_pv_tuning.gemm_cus;
    if (n <= 0) {
        static std::atomic<int> per_dev[64];
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
        n = per_dev[dev].load(std::memory_order_relaxed);
        if (n == 0) {
            hipDeviceProp_t prop;
            n = hipGetDeviceProperties(&prop, dev) == hipSuccess ? prop.multiProcessorCount : 256;
            if (n <= 0) n = 256;
            per_dev[dev].store(n, std::memory_order_relaxed);
        }
    }
    n -= n % 8;
    return n <= 0 ? 8 : n;
}

// v4 or v7 for this shape?  Cost model = rounds over the chip x time of one round, the round times being the
// measured per-tile K-loop + epilogue of the two kernels at K = 768 on the B/32 shapes (tools/gemm_trace.py):
// v4 25 us for 3 x (128 x 128) per CU, v7 26.5 us (MB = 4) / 32 us (MB = 5) for one (64*MB) x 256 per CU.
inline int pick_v7(const GemmParams& p) {
    if (g_pv_tuning.gemm_tile >= 0) return g_pv_tuning.gemm_tile;           // 0 = v4, 4 / 5 = v7<MB>
    auto rounds = [](int64_t tiles, int64_t slots) { return (double)((tiles + slots - 1) / slots); };
    const int64_t M = p.M, N = p.N, cus = pv_gemm_cus(p);
    // (the round times predate the full-line loop, which makes the v7 tiles about 10 % faster; scaling them moved only the
    // 512 x 512 head GEMM from 16 small tiles to 4 large ones -- slower -- so the measured constants stay)
    const double c4 = rounds(((M + 127) / 128) * ((N + 127) / 128), 3 * cus) * 25.0;
    const double c74 = rounds(((M + 255) / 256) * ((N + 255) / 256), cus) * 26.5;
    const double c75 = rounds(((M + 319) / 320) * ((N + 255) / 256), cus) * 32.0;
    if (c4 <= c74 && c4 <= c75) return 0;
    return c75 <= c74 ? 5 : 4;
}

// THE decision: which kernel this launch gets, in which form, on which grid.  Everything that launches or describes a GEMM reads it
// from here (pv_launch_gemm, its trace info).  Precedence: [K][N] B operand -> gemm_kernel; plain A with 16-byte-legal operands
// inside the 32-bit span limits -> v4, or (bf16, vector epilogue, N % 8 == 0, residual rows in 32-bit reach) what pick_v7 says;
// bf16 patch gather at patch size 32 -> v7 if pick_v7 says so; everything else -> gemm_kernel.
// Tuning keys: gemm_v1, gemm_v1patch, gemm_tile, gemm_loop, gemm_persist.
GemmChoice choose(int dtype, const GemmParams& p) {
    const int EB = dtype == PV_DTYPE_BF16 ? 2 : 4;
    GemmChoice c{};
    c.kernel = PV_GEMM_GENERIC;
    c.tm = BM;
    c.tn = BN;
    bool tiled = false;          // bf16 and legal for the tiled family: pick_v7 has the word
    if (p.b_kn) {
        // (pv_launch_gemm has required fp32, plain A and 16-byte-legal operands)
        c.vec = true;
        c.vec_out = (p.ldo * 4) % 16 == 0 && pv_aligned16(p.out0) && pv_aligned16(p.out1) && pv_aligned16(p.bias0);
    } else {
        const bool kvec = ((int64_t)p.K * EB) % 16 == 0;
        const bool b_vec = kvec && (p.ldb * EB) % 16 == 0 && pv_aligned16(p.Bt);
        bool a_vec;
        if (p.a_mode == PV_A_PLAIN) {
            a_vec = kvec && (p.lda * EB) % 16 == 0 && pv_aligned16(p.A);
        } else {
            a_vec = (p.pP * EB) % 16 == 0 && (p.pS * EB) % 16 == 0 && pv_aligned16(p.A);
        }
        const bool vec = a_vec && b_vec;
        // vector epilogue legality
        bool vo = (p.ldo * EB) % 16 == 0 && pv_aligned16(p.out0) && pv_aligned16(p.out1) && pv_aligned16(p.out2) &&
                  pv_aligned16(p.bias0) && pv_aligned16(p.bias1) && pv_aligned16(p.bias2);
        if (p.epi == PV_EPI_RESID) vo = vo && (p.ldr * EB) % 16 == 0 && pv_aligned16(p.resid);
        if (p.epi == PV_EPI_QKV) vo = vo && (p.nsplit % 8) == 0;
        c.vec = vec;
        c.vec_out = vo;
        const uint64_t spanA = ((uint64_t)p.M + BM) * (uint64_t)p.lda * EB, spanB = ((uint64_t)p.N + BN) * (uint64_t)p.ldb * EB;
        if (p.a_mode == PV_A_PLAIN && vec && spanA < 0xffffff00ull && spanB < 0xffffff00ull && !g_pv_tuning.gemm_v1) {
            // 128 x 128 tiles, 3 workgroups / CU (v4) or one 8-wave workgroup with a (64*MB) x 256 tile (v7);
            // history and measurements of the variants in between: profiles/r01_notes.md
            c.kernel = PV_GEMM_V4;
            // (the residual park addresses a wave's 160 residual rows with 32-bit offsets)
            const bool r_ok = p.epi != PV_EPI_RESID || (uint64_t)p.ldr * EB * 320 < 0xffffff00ull;
            tiled = EB == 2 && vo && p.N % 8 == 0 && r_ok;
        } else if (EB == 2 && p.a_mode == PV_A_PATCH) {
            // patch embedding at patch size 32: the tiled kernel gathers the patches itself (see gemm_kernel_v7)
            const uint64_t img_bytes = (uint64_t)(p.pG ? p.M / (p.pG * p.pG) : 0) * p.pC * p.pS * p.pS * EB;
            tiled = vec && vo && p.N % 8 == 0 && p.pP == 32 && p.K == p.pC * 1024 && p.pG > 0 && p.M % (p.pG * p.pG) == 0 &&
                    img_bytes < 0xffffff00ull && (uint64_t)(p.N + 256) * p.ldb * EB < 0xffffff00ull && !g_pv_tuning.gemm_v1 &&
                    !g_pv_tuning.gemm_v1patch;
        }
    }
    const int pick = tiled ? pick_v7(p) : 0;
    if (pick == 4 || pick == 5) {
        c.kernel = PV_GEMM_V7;
        c.MB = pick;
        c.tm = 64 * pick;
        c.tn = 256;
    }
    c.ntiles = ((p.M + c.tm - 1) / c.tm) * ((p.N + c.tn - 1) / c.tn);
    c.grid = c.ntiles;
    if (c.kernel == PV_GEMM_V7) {
        // K loop: 2 = full-line form (whole 128-byte slabs: every B/32, L/14 shape), 1 = pipelined 64-byte slabs (plain A operands,
        // whole 64-byte slabs), 0 = the barrier-then-fetch loop (patch gather, K tails).  gemm_loop: -1 auto, 0 / 1 force the
        // simpler forms where legal.
        const int64_t kbytes = (int64_t)p.K * EB;
        if (p.a_mode == PV_A_PLAIN && kbytes % 64 == 0 && g_pv_tuning.gemm_loop != 0)
            c.LP = (kbytes % 128 == 0 && g_pv_tuning.gemm_loop != 1) ? 2 : 1;
        // persistent form (v8): the full-line loop's shapes with an even slab count, when the launch has more tiles than CUs
        // (gemm_persist: -1 auto, 0 never, 1 wherever legal)
        const int n_cu = pv_gemm_cus(p);
        if (c.LP == 2 && (kbytes / 128) % 2 == 0 && g_pv_tuning.gemm_persist != 0 && (g_pv_tuning.gemm_persist > 0 || c.ntiles > n_cu)) {
            c.kernel = PV_GEMM_V8;
            c.grid = c.ntiles < n_cu ? c.ntiles : n_cu;
        }
    }
    return c;
}

// debug tracing (pv_debug_gemm_trace_*; the stamps are written by trace_stamp, gemm_epi.hpp)
uint64_t* g_trace_dev = nullptr;
int g_trace_countdown = -1;
int32_t g_trace_info[6] = {0, 0, 0, 0, 0, 0};
constexpr int TRACE_MAX_WG = 8192;
}  // namespace

extern "C" int pv_debug_gemm_trace_arm(int32_t launch_idx) {
    if (!g_trace_dev) {
        PV_HIP_CHECK(hipMalloc(&g_trace_dev, (size_t)TRACE_MAX_WG * 4 * sizeof(uint64_t)));
    }
    PV_HIP_CHECK(hipMemset(g_trace_dev, 0, (size_t)TRACE_MAX_WG * 4 * sizeof(uint64_t)));
    g_trace_countdown = launch_idx;
    return PV_OK;
}

extern "C" int pv_debug_gemm_trace_read(uint64_t* host_out, int32_t max_wg, int32_t* info6) {
    PV_REQUIRE(g_trace_dev && host_out && info6, "trace not armed");
    PV_HIP_CHECK(hipDeviceSynchronize());
    const int n = max_wg < g_trace_info[4] ? max_wg : g_trace_info[4];
    PV_HIP_CHECK(hipMemcpy(host_out, g_trace_dev, (size_t)n * 4 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    for (int i = 0; i < 6; ++i) info6[i] = g_trace_info[i];
    return PV_OK;
}

int pv_launch_gemm(int dtype, GemmParams p, hipStream_t stream) {
    // instance tag for the per-instance roofline (bench.py): 1 QKV, 2 O-projection, 3 MLP-1, 4 MLP-2, 0 everything else
    struct TagScope { TagScope(int t) { pv_prof_set_tag(t); } ~TagScope() { pv_prof_set_tag(0); } }
        tag_scope(p.epi == PV_EPI_QKV ? 1 : p.epi == PV_EPI_ACT ? 3 : p.epi == PV_EPI_RESID ? (p.K > p.N ? 4 : 2) : 0);
    p.dbg = g_pv_tuning.gemm_dbg;
    p.trace = nullptr;
    PV_REQUIRE(p.M > 0 && p.N > 0 && p.K > 0, "gemm dims must be positive");
    PV_REQUIRE(p.A && p.Bt, "gemm operands must be non-null");
    if (p.epi == PV_EPI_BIAS) PV_REQUIRE(p.out0, "EPI_BIAS needs out0");
    if (p.epi == PV_EPI_QKV) PV_REQUIRE(p.out0 && p.out1 && p.out2 && p.nsplit > 0 && p.N == 3 * p.nsplit, "EPI_QKV outputs");
    if (p.epi == PV_EPI_RESID) PV_REQUIRE(p.out1 && p.resid, "EPI_RESID needs out1 and resid");
    if (p.epi == PV_EPI_ACT) PV_REQUIRE(p.out1, "EPI_ACT needs out1");
    if (p.b_kn) {
        PV_REQUIRE(dtype == PV_DTYPE_F32 && p.a_mode == PV_A_PLAIN, "[K][N] B operand: fp32, plain A only");
        PV_REQUIRE(p.N % 4 == 0 && p.ldb % 4 == 0 && pv_aligned16(p.Bt), "[K][N] B operand alignment");
        PV_REQUIRE(((int64_t)p.K * 4) % 16 == 0 && (p.lda * 4) % 16 == 0 && pv_aligned16(p.A), "[K][N] path needs 16-byte aligned A rows");
    }
    if (dtype != PV_DTYPE_BF16 && dtype != PV_DTYPE_F32) {
        pv_set_error("gemm: unsupported dtype");
        return PV_ERR_INVALID;
    }
    const GemmChoice c = choose(dtype, p);
    p.vec_out = c.vec_out ? 1 : 0;
    if (g_trace_countdown >= 0 && p.a_mode == PV_A_PLAIN && !p.b_kn) {
        if (g_trace_countdown-- == 0) {
            // info = {M, N, K, epi, workgroups that stamp, kernel}: 70 + MB for v7 / v8 (v8 stamps per virtual block id: one row
            // per tile), 4 for v4; gemm_kernel writes no stamps: kernel 1, no workgroups, and it is not handed the buffer
            const bool stamps = c.kernel != PV_GEMM_GENERIC;
            g_trace_info[0] = p.M; g_trace_info[1] = p.N; g_trace_info[2] = p.K; g_trace_info[3] = p.epi;
            g_trace_info[4] = stamps ? c.ntiles : 0;
            g_trace_info[5] = c.MB ? 70 + c.MB : c.kernel;
            if (stamps && c.ntiles <= TRACE_MAX_WG) p.trace = g_trace_dev;
        }
    }
    switch (c.kernel) {
        case PV_GEMM_V7:
        case PV_GEMM_V8: return pv_gemm_launch_tiled(p, c, stream);
        case PV_GEMM_V4: return pv_gemm_launch_v4(dtype, p, c, stream);
        default: return pv_gemm_launch_generic(dtype, p, c, stream);
    }
}
