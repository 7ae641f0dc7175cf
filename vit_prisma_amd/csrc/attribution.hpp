// What the two attribution files share: the by-value pointer table of the L taps / weights, the tile constants of attr_fold_kernel
// and the host launcher of that kernel.  The kernel itself stays in attribution.hip; attribution_neuron.hip folds mlp.W_out
// ([d_mlp, d_model] row-major bf16) through the same launcher with HD = d_mlp.
#pragma once
#include "pv_common.hpp"

struct AttrPtrs {
    const void* ptr[PV_ATTR_MAX_LAYERS];
};

constexpr int FOLD_TJ = 64, FOLD_TR = 16, FOLD_KC = 64, FOLD_WS = FOLD_KC + 4;   // W rows padded to 68 floats: 16-byte aligned, spread over the banks

// attribution.hip: G[l, r, j] = sum_k W_l[j, k] (a[r, k] - mean_k a[r, :]) for the n_layers row-major bf16 [HD, d_model] matrices W
// (HOST array of device pointers) and the R fp32 answer rows, into G fp32 [n_layers, R, HD].  `who` starts the error text
// ("head attribution", "neuron attribution").  Nothing is allocated; the caller has checked the pointers and d_model % 8 == 0.
int attr_launch_fold(const char* who, const void* const* W, int n_layers, int64_t HD, int d_model, int64_t R, const float* answers,
                     float* G, hipStream_t stream);
