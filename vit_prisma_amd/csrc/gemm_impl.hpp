// Internal to the GEMM sources: GemmChoice and the launchers.  gemm.hip decides which kernel a launch gets (choose()); the kernel
// files (gemm_generic.hip, a translation unit of its own; gemm_v4.hpp and gemm_tiled.hpp, which gemm.hip includes) keep their kernels
// in anonymous namespaces and define one launcher each, which launches what was decided.
#pragma once
#include "gemm.hpp"

namespace {
// the tile of gemm_kernel and gemm_kernel_v4 (and the slack of the 32-bit span limits in choose())
constexpr int BM = 128;
constexpr int BN = 128;
}  // namespace

enum { PV_GEMM_GENERIC = 1, PV_GEMM_V4 = 4, PV_GEMM_V7 = 7, PV_GEMM_V8 = 8 };

// what choose() decided for one launch
struct GemmChoice {
    int kernel;          // PV_GEMM_*: gemm_kernel, gemm_kernel_v4, gemm_kernel_v7, gemm_kernel_v8
    int MB;              // v7 / v8: the tile is (64*MB) x 256, MB = 4 | 5; 0 for the others
    int LP;              // v7: K-loop form, 0 barrier-then-fetch, 1 pipelined 64-byte slabs, 2 full-line (v8 is always 2)
    bool vec;            // gemm_kernel: 16-byte operand loads are legal
    bool vec_out;        // 16-byte vector epilogue is legal (becomes GemmParams::vec_out)
    int tm, tn;          // tile shape
    int ntiles;          // tiles of the output = workgroups of the launch, except for v8
    int grid;            // workgroups launched (v8: min(ntiles, CUs); each walks the virtual block ids bid, bid + grid, .. < ntiles)
};

// p.vec_out is set from the choice by the caller.  Return PV_OK / error code.
int pv_gemm_launch_generic(int dtype, const GemmParams& p, const GemmChoice& c, hipStream_t stream);
int pv_gemm_launch_v4(int dtype, const GemmParams& p, const GemmChoice& c, hipStream_t stream);
int pv_gemm_launch_tiled(const GemmParams& p, const GemmChoice& c, hipStream_t stream);      // bf16 only
