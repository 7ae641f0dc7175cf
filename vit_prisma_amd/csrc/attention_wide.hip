// Attention core for wide heads, 64 < d_head <= 128 with d_head % 8 == 0 (CLIP ViT-H/14: 80, g/14: 88, bigG/14: 104), every
// T <= PV_ATTN_MAX_TOKENS, fp32 and bf16: attn_stream_body (attn_stream.hpp) at its ragged width.  The kernel is compiled per padded
// width DHP (96 for d_head 72 - 96, 128 for 104 - 128), the true d_head is a run-time value, and columns d_head .. DHP - 1 contribute
// exact zeros (the rules are with the body).
// LDS: <float, 96> 82.0 KiB, <float, 128> 98.0 KiB, <bf16, 96> 60.0 KiB, <bf16, 128> 69.0 KiB.  Stated floor
// (tests/test_wide_heads_cpu.py): 1 wave per SIMD for the fp32 instances (z alone is 48 / 64 accumulator registers), 2 for the bf16
// ones; no scratch.
#include "attention.hpp"

#include "attn_stream.hpp"

namespace {

template <typename E, int DHP>
__global__ __launch_bounds__(256, sizeof(E) == 4 ? 1 : 2) void attn_wide_kernel(const AttnParams p) {
    static_assert(DHP == 96 || DHP == 128, "padded d_head 96 / 128");
    attn_stream_body<E, DHP, true, false>(p);
}

template <typename E>
int launch_wide(const AttnParams& p, hipStream_t stream) {
    return p.dh <= 96 ? launch_attn_streaming<E>(attn_wide_kernel<E, 96>, "attn_wide_kernel", p, stream)
                      : launch_attn_streaming<E>(attn_wide_kernel<E, 128>, "attn_wide_kernel", p, stream);
}

}  // namespace

int pv_attention_wide_supported(int dh) { return (dh > 64 && dh <= 128 && dh % 8 == 0) ? 1 : 0; }

int pv_launch_attention_wide(int dtype, const AttnParams& p, hipStream_t stream) {
    PV_REQUIRE(pv_attention_wide_supported(p.dh) && p.T >= 1 && p.T <= PV_ATTN_MAX_TOKENS,
               "attention: unsupported (T, d_head); supported: T <= " PV_STR(PV_ATTN_MAX_TOKENS)
               ", d_head in {32, 64} or 64 < d_head <= 128 with d_head % 8 == 0");
    if (dtype == PV_DTYPE_BF16) return launch_wide<bf16_t>(p, stream);
    if (dtype == PV_DTYPE_F32) return launch_wide<float>(p, stream);
    pv_set_error("attention: unsupported dtype");
    return PV_ERR_INVALID;
}
