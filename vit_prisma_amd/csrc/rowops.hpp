#pragma once
#include "pv_common.hpp"

struct LnParams {
    const void* x;        // [rows][ldx] T  (EMBED: patch embeddings [B*(T-cls)][d])
    int64_t ldx;
    const void* w;        // [d] T
    const void* b;        // [d] T
    int32_t rows, d;
    float eps;
    float* scale_out;     // [rows] fp32 or NULL                      (hook_scale)
    float* norm_f32_out;  // [rows][d] fp32 or NULL (bf16 mode tap)   (hook_normalized)
    void* out;            // [rows][d] T or NULL                      (LN output in storage dtype)
    // embed-assembly mode
    int32_t embed;        // 1: build rows from cls/patch + pos
    int32_t do_ln;        // 0: only assemble (layer_norm_pre == False)
    int32_t T;            // tokens per image
    int32_t use_cls;
    const void* cls;      // [d] T
    const void* pos;      // [T][d] T
    void* full_out;       // [rows][d] T or NULL                      (hook_full_embed)
};

int pv_launch_ln(int dtype, const LnParams& p, hipStream_t stream);
// out[i] = T(in[i]) (round to the storage dtype; a plain copy in fp32 mode): the LayerNorm output rebuilt from an edited
// hook_normalized tensor (pv_vit_forward_stage, PV_STAGE_LN1 / PV_STAGE_LN2).  n % 4 == 0.
int pv_launch_cast_from_f32(int dtype, const float* in, void* out, int64_t n, hipStream_t stream);
int pv_launch_l2norm(int dtype, const void* x, void* out, int rows, int n, hipStream_t stream);
// x [B][T][d] (the ln_final output) -> mean over tokens t0 .. T - 1, fp32 accumulation, one rounding (models/base_vit.py:195-208):
// pair == 0: out [B][d] ("gaap" with t0 = 0); pair == 1: out [B][d][2] = (x[b][0][c], mean) -- the dino-vitb output (t0 = 1)
int pv_launch_token_mean(int dtype, const void* x, void* out, int B, int T, int d, int t0, int pair, hipStream_t stream);
// The text tower's embedding (models/base_text_transformer.py:139-145): tokens [B][T] int64, W_E [vocab][d], pos [T][d] ->
// embed_out [B][T][d] = W_E[tokens] (bit-exact gather) and full_out = round_T(embed + pos); either may be NULL.  An id outside
// [0, vocab) reads no memory: its rows are NaN.
int pv_launch_token_embed(int dtype, const int64_t* tokens, const void* W_E, const void* pos, void* embed_out, void* full_out, int B,
                          int T, int d, int vocab, hipStream_t stream);
// out [B][d] = x[b][first argmax_t tokens[b][t]] (base_text_transformer.py:151); x [B][T][d]
int pv_launch_eot_rows(int dtype, const int64_t* tokens, const void* x, void* out, int B, int T, int d, hipStream_t stream);
int pv_launch_transpose(int elem_bytes, const void* in, void* out, int batch, int R, int C, hipStream_t stream);
// bf16 NCHW images -> [B*G*G][Kp] patch rows (im2col once per batch, zero-padded to Kp columns), and the matching row padding
// of the [d][K] patch-embedding weights: the operands of the tiled GEMM for patch sizes its in-kernel gather does not cover
int pv_launch_patch_pack_bf16(const void* images, void* out, int B, int C, int S, int p, int G, int Kp, hipStream_t stream);
int pv_launch_pad_rows_bf16(const void* in, void* out, int R, int K, int Kp, hipStream_t stream);
