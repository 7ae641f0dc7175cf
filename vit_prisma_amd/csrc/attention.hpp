#pragma once
#include "pv_common.hpp"

struct AttnParams {
    const void *q, *k, *v;     // [B, T, H, dh] T
    void* scores;              // [B, H, T, T] T or NULL (tap)
    void* pattern;             // [B, H, T, T] T or NULL (tap)
    void* z;                   // [B, T, H, dh] T
    int32_t B, T, H, dh;
    float attn_scale;
    int32_t Tpad;              // filled by the launcher
    int32_t causal;            // != 0: scores + (-inf where key > query) (the text tower); d_head 32 / 64 only
};

int pv_attention_supported(int T, int dh);
int pv_launch_attention(int dtype, AttnParams p, hipStream_t stream);
// Wide heads, 64 < d_head <= 128 with d_head % 8 == 0 (attention_wide.hip): pv_launch_attention sends them here at every T.
int pv_attention_wide_supported(int dh);
int pv_launch_attention_wide(int dtype, const AttnParams& p, hipStream_t stream);
// Causal attention, p.causal != 0 (attention_causal.hip): d_head 32 / 64, 1 <= T <= PV_ATTN_MAX_TOKENS, both dtypes;
// pv_launch_attention sends every causal call here before its non-causal table.
int pv_launch_attention_causal(int dtype, const AttnParams& p, hipStream_t stream);
// The attention core resumed behind a hooked activation (pv_vit_forward_stage, PV_STAGE_SCORES / PV_STAGE_PATTERN):
// from_scores: p.scores is the INPUT (the edited hook_attn_scores tensor): pattern = softmax, NaN -> 0 (attention.py:148-150),
// written to p.pattern when non-NULL, z = pattern v; otherwise p.pattern is the INPUT (the edited hook_pattern tensor) and
// z = pattern v.  q / k are unused.  A simple one-wave-per-query-row kernel: interventions, not the all-hooks hot path.
int pv_launch_attention_resume(int dtype, AttnParams p, int from_scores, hipStream_t stream);
