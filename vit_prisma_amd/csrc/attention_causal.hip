// Causal attention core of the text tower (HookedTextTransformer: models/base_text_transformer.py:188-194 builds the mask, -inf above
// the diagonal, and models/layers/attention.py:262-265 adds it to the scaled scores): attn_stream_body (attn_stream.hpp) with
// CAUSAL = true, d_head 32 / 64, every 1 <= T <= PV_ATTN_MAX_TOKENS (CLIP's context is 77), fp32 and bf16.  A kernel of its own name:
// the non-causal kernels keep their code and their names.  LDS and launch bounds are attn_stream_kernel's; stated floor
// (tests/test_text_kernel_resources_cpu.py): 2 waves per SIMD for <float, 64>, 3 for the other three instances; no scratch.
// Prompts are encoded once per class list, so this path is not tuned for T = 77: whether a masked attn_lean_kernel would be faster
// there in bf16 has not been measured.
#include "attention.hpp"

#include "attn_stream.hpp"

namespace {

template <typename E, int DH>
__global__ __launch_bounds__(256, (sizeof(E) == 4 && DH == 64) ? 2 : 3) void attn_causal_kernel(const AttnParams p) {
    static_assert(DH == 32 || DH == 64, "d_head 32 / 64");
    attn_stream_body<E, DH, false, true>(p);
}

template <typename E>
int launch_causal(const AttnParams& p, hipStream_t stream) {
    return p.dh == 64 ? launch_attn_streaming<E>(attn_causal_kernel<E, 64>, "attn_causal_kernel", p, stream)
                      : launch_attn_streaming<E>(attn_causal_kernel<E, 32>, "attn_causal_kernel", p, stream);
}

}  // namespace

int pv_launch_attention_causal(int dtype, const AttnParams& p, hipStream_t stream) {
    PV_REQUIRE((p.dh == 32 || p.dh == 64) && p.T >= 1 && p.T <= PV_ATTN_MAX_TOKENS,
               "causal attention: supported: d_head in {32, 64} and 1 <= T <= " PV_STR(PV_ATTN_MAX_TOKENS)
               "; the wide heads (64 < d_head <= 128) have no causal kernel");
    if (dtype == PV_DTYPE_BF16) return launch_causal<bf16_t>(p, stream);
    if (dtype == PV_DTYPE_F32) return launch_causal<float>(p, stream);
    pv_set_error("attention: unsupported dtype");
    return PV_ERR_INVALID;
}
