// Host-side plan + launch sequence of the tapped ViT forward (C ABI in include/pv_native.h).
// Mirrors HookedViT.forward (/root/reference/src/vit_prisma/models/base_vit.py:152-217) and
// TransformerBlock.forward (models/layers/transformer_block.py:80-138); ln1 is evaluated ONCE per
// block (the reference evaluates it three times with identical results, :106-109).
#include <string.h>

#include <vector>

#include "attention.hpp"
#include "gemm.hpp"
#include "rowops.hpp"

static thread_local std::string g_last_error;
void pv_set_error(const std::string& msg) { g_last_error = msg; }

extern "C" int pv_abi_version(void) { return PV_ABI_VERSION; }
extern "C" void pv_last_error(char* buf, size_t len) {
    if (!buf || len == 0) return;
    strncpy(buf, g_last_error.c_str(), len - 1);
    buf[len - 1] = 0;
}

struct LayerShadow {
    unsigned char* Wqkv;   // [3*H*dh][d]
    unsigned char* WoT;    // [d][H*dh]
    unsigned char* WinT;   // [d_mlp][d]
    unsigned char* WoutT;  // [d][d_mlp]
};

struct pv_vit_plan {
    pv_vit_desc d;
    int P, G, T, HD, EB;
    pv_vit_weights w;
    std::vector<pv_vit_layer_weights> lw;
    std::vector<LayerShadow> sh;
    unsigned char* WhT;
    // bf16, even patch size other than 32: the patches are packed into GEMM rows once per batch (Kp = K rounded up to 8
    // columns) so that the patch embedding runs on the tiled DMA GEMM instead of the register-staged gather kernel
    // (L/14@336: 1.06 ms -> pack + GEMM); conv_wp = the weights padded to Kp columns (the parameter itself when Kp == K)
    bool patch_prepack;
    int Kp;
    unsigned char* conv_wp;
    bool weights_set;
    // a text plan (pv_text_plan_create): d holds the shared fields (n_tokens = context_length, PV_POOL_CLS stands for the EOT row),
    // P == T sizes the hook_embed buffer, and the embedding tables replace the patch weights
    bool is_text;
    int vocab, causal;
    const void *token_embed, *pos_embed;
};

static size_t seg(size_t elems, int eb) { return (size_t)pv_align_up((int64_t)elems * eb, 256); }

static pv_vit_plan* new_plan(const pv_vit_desc& d, int G, int P) {
    pv_vit_plan* p = new pv_vit_plan();
    p->d = d;
    p->G = G;
    p->P = P;
    p->T = d.n_tokens;
    p->HD = d.n_heads * d.d_head;
    p->EB = d.dtype == PV_DTYPE_BF16 ? 2 : 4;
    p->WhT = nullptr;
    p->conv_wp = nullptr;
    p->Kp = 0;
    p->patch_prepack = false;
    p->weights_set = false;
    p->is_text = false;
    p->vocab = 0;
    p->causal = 0;
    p->token_embed = p->pos_embed = nullptr;
    return p;
}

extern "C" int pv_vit_plan_create(const pv_vit_desc* desc, pv_vit_plan** out_plan) {
    PV_REQUIRE(desc && out_plan, "null argument");
    const pv_vit_desc& d = *desc;
    PV_REQUIRE(d.dtype == PV_DTYPE_F32 || d.dtype == PV_DTYPE_BF16, "dtype must be fp32 or bf16");
    PV_REQUIRE(d.n_layers >= 0 && d.d_model > 0 && d.n_heads > 0 && d.d_head > 0 && d.d_mlp > 0, "dims");
    PV_REQUIRE(d.d_model % 8 == 0 && d.d_model <= 2048, "d_model must be a multiple of 8 and <= 2048");
    PV_REQUIRE(d.d_mlp % 8 == 0, "d_mlp must be a multiple of 8");
    PV_REQUIRE(d.patch_size > 0 && d.image_size >= d.patch_size, "patch/image size");
    const int G = d.image_size / d.patch_size;
    const int P = G * G;
    PV_REQUIRE(d.n_tokens == P + (d.use_cls_token ? 1 : 0), "n_tokens != patches (+cls)");
    PV_REQUIRE(pv_attention_supported(d.n_tokens, d.d_head), "attention shape unsupported (T <= " PV_STR(PV_ATTN_MAX_TOKENS) ", d_head in {32, 64} or 64 < d_head <= 128 with d_head % 8 == 0)");
    PV_REQUIRE(d.pooling >= PV_POOL_CLS && d.pooling <= PV_POOL_CLS_MEAN, "pooling");
    // cat(cls, mean(patches)) is [B, d_model, 2]: the reference's registry has it without a head only (base_vit.py:199-208)
    PV_REQUIRE(d.pooling != PV_POOL_CLS_MEAN || (!d.has_head && d.n_tokens >= 2), "PV_POOL_CLS_MEAN needs has_head == 0 and a patch token");
    PV_REQUIRE(d.activation >= PV_ACT_GELU && d.activation <= PV_ACT_RELU, "activation");
    if (d.has_head) PV_REQUIRE(d.n_classes > 0, "n_classes");
    pv_vit_plan* p = new_plan(d, G, P);
    p->Kp = (d.n_channels * d.patch_size * d.patch_size + 7) / 8 * 8;
    p->patch_prepack = d.dtype == PV_DTYPE_BF16 && d.patch_size != 32 && d.patch_size % 2 == 0 && d.image_size % 2 == 0;
    *out_plan = p;
    return PV_OK;
}

extern "C" int pv_text_plan_create(const pv_text_desc* desc, pv_vit_plan** out_plan) {
    PV_REQUIRE(desc && out_plan, "null argument");
    const pv_text_desc& t = *desc;
    PV_REQUIRE(t.dtype == PV_DTYPE_F32 || t.dtype == PV_DTYPE_BF16, "dtype must be fp32 or bf16");
    PV_REQUIRE(t.n_layers >= 0 && t.d_model > 0 && t.n_heads > 0 && t.d_head > 0 && t.d_mlp > 0 && t.vocab_size > 0, "dims");
    PV_REQUIRE(t.d_model % 8 == 0 && t.d_model <= 2048, "d_model must be a multiple of 8 and <= 2048");
    PV_REQUIRE(t.d_mlp % 8 == 0, "d_mlp must be a multiple of 8");
    PV_REQUIRE(t.context_length >= 1 && t.context_length <= PV_ATTN_MAX_TOKENS, "context_length must be in [1, " PV_STR(PV_ATTN_MAX_TOKENS) "]");
    if (t.causal) PV_REQUIRE(t.d_head == 32 || t.d_head == 64, "causal attention needs d_head in {32, 64} (the wide heads have no causal kernel)");
    else PV_REQUIRE(pv_attention_supported(t.context_length, t.d_head), "attention shape unsupported (T <= " PV_STR(PV_ATTN_MAX_TOKENS) ", d_head in {32, 64} or 64 < d_head <= 128 with d_head % 8 == 0)");
    PV_REQUIRE(t.activation >= PV_ACT_GELU && t.activation <= PV_ACT_RELU, "activation");
    if (t.has_head) PV_REQUIRE(t.n_classes > 0, "n_classes");
    pv_vit_desc d = {};
    d.n_layers = t.n_layers; d.d_model = t.d_model; d.n_heads = t.n_heads; d.d_head = t.d_head; d.d_mlp = t.d_mlp;
    d.n_tokens = t.context_length; d.n_classes = t.n_classes; d.has_head = t.has_head; d.normalize_output = t.normalize_output;
    d.activation = t.activation; d.dtype = t.dtype; d.eps = t.eps; d.attn_scale = t.attn_scale; d.pooling = PV_POOL_CLS;
    pv_vit_plan* p = new_plan(d, 0, t.context_length);
    p->is_text = true;
    p->vocab = t.vocab_size;
    p->causal = t.causal ? 1 : 0;
    *out_plan = p;
    return PV_OK;
}

extern "C" void pv_vit_plan_destroy(pv_vit_plan* plan) { delete plan; }

extern "C" size_t pv_vit_shadow_bytes(const pv_vit_plan* p) {
    if (!p) return 0;
    const pv_vit_desc& d = p->d;
    size_t per_layer = seg((size_t)3 * p->HD * d.d_model, p->EB) + seg((size_t)d.d_model * p->HD, p->EB) +
                       2 * seg((size_t)d.d_model * d.d_mlp, p->EB);
    size_t total = per_layer * d.n_layers;
    if (d.has_head) total += seg((size_t)d.n_classes * d.d_model, p->EB);
    if (p->patch_prepack) total += seg((size_t)d.d_model * p->Kp, p->EB);
    return total + 256;
}

// the shadows both kinds of plan share: per layer Wqkv, WoT, WinT, WoutT, then the head's; `cur` is left behind the last one
static int pack_block_and_head_shadows(pv_vit_plan* p, const pv_vit_layer_weights* layers, const void* W_H, unsigned char*& cur,
                                       hipStream_t stream) {
    const pv_vit_desc& d = p->d;
    p->lw.assign(layers, layers + d.n_layers);
    p->w.layers = p->lw.data();
    p->sh.resize(d.n_layers);
    const int EB = p->EB, HD = p->HD, dm = d.d_model, dmlp = d.d_mlp, H = d.n_heads, dh = d.d_head;
    for (int l = 0; l < d.n_layers; ++l) {
        const pv_vit_layer_weights& L = p->lw[l];
        PV_REQUIRE(L.ln1_w && L.ln1_b && L.W_Q && L.W_K && L.W_V && L.b_Q && L.b_K && L.b_V && L.W_O && L.b_O &&
                       L.ln2_w && L.ln2_b && L.W_in && L.b_in && L.W_out && L.b_out,
                   "missing block weights");
        LayerShadow& S = p->sh[l];
        S.Wqkv = cur; cur += seg((size_t)3 * HD * dm, EB);
        S.WoT = cur;  cur += seg((size_t)dm * HD, EB);
        S.WinT = cur; cur += seg((size_t)dm * dmlp, EB);
        S.WoutT = cur; cur += seg((size_t)dm * dmlp, EB);
        // W_Q[h][k][e] -> Wqkv[(h*dh+e)][k]   (attention.py:216-220: x @ W[h] + b[h])
        int rc;
        if ((rc = pv_launch_transpose(EB, L.W_Q, S.Wqkv, H, dm, dh, stream))) return rc;
        if ((rc = pv_launch_transpose(EB, L.W_K, S.Wqkv + (size_t)HD * dm * EB, H, dm, dh, stream))) return rc;
        if ((rc = pv_launch_transpose(EB, L.W_V, S.Wqkv + (size_t)2 * HD * dm * EB, H, dm, dh, stream))) return rc;
        // W_O[h][e][n] == [K = h*dh+e][N = d] -> [N][K]   (attention.py:155-167)
        if ((rc = pv_launch_transpose(EB, L.W_O, S.WoT, 1, HD, dm, stream))) return rc;
        if ((rc = pv_launch_transpose(EB, L.W_in, S.WinT, 1, dm, dmlp, stream))) return rc;
        if ((rc = pv_launch_transpose(EB, L.W_out, S.WoutT, 1, dmlp, dm, stream))) return rc;
    }
    if (d.has_head) {
        p->WhT = cur;
        cur += seg((size_t)d.n_classes * dm, EB);
        int rc;
        if ((rc = pv_launch_transpose(EB, W_H, p->WhT, 1, dm, d.n_classes, stream))) return rc;
    }
    return PV_OK;
}

extern "C" int pv_text_plan_set_weights(pv_vit_plan* p, const pv_text_weights* w, void* shadow, size_t shadow_bytes, void* stream_) {
    PV_REQUIRE(p && w && shadow, "null argument");
    PV_REQUIRE(p->is_text, "pv_text_plan_set_weights needs a plan of pv_text_plan_create");
    PV_REQUIRE(shadow_bytes >= pv_vit_shadow_bytes(p), "shadow buffer too small");
    PV_REQUIRE(((uintptr_t)shadow & 255) == 0, "shadow buffer must be 256-byte aligned");
    const pv_vit_desc& d = p->d;
    PV_REQUIRE(w->token_embed && w->pos_embed && w->ln_final_w && w->ln_final_b, "missing global weights");
    PV_REQUIRE(pv_aligned16(w->token_embed) && pv_aligned16(w->pos_embed), "token_embed / pos_embed must be 16-byte aligned");
    if (d.has_head) PV_REQUIRE(w->W_H && w->b_H, "missing head weights");
    PV_REQUIRE(d.n_layers == 0 || w->layers, "missing layer weights");
    p->w = pv_vit_weights{};
    p->w.ln_final_w = w->ln_final_w; p->w.ln_final_b = w->ln_final_b; p->w.W_H = w->W_H; p->w.b_H = w->b_H;
    p->token_embed = w->token_embed;
    p->pos_embed = w->pos_embed;
    unsigned char* cur = (unsigned char*)shadow;
    int rc;
    if ((rc = pack_block_and_head_shadows(p, w->layers, w->W_H, cur, (hipStream_t)stream_))) return rc;
    p->weights_set = true;
    return PV_OK;
}

extern "C" int pv_vit_plan_set_weights(pv_vit_plan* p, const pv_vit_weights* w, void* shadow,
                                       size_t shadow_bytes, void* stream_) {
    PV_REQUIRE(p && w && shadow, "null argument");
    PV_REQUIRE(!p->is_text, "a text plan takes its weights through pv_text_plan_set_weights");
    PV_REQUIRE(shadow_bytes >= pv_vit_shadow_bytes(p), "shadow buffer too small");
    PV_REQUIRE(((uintptr_t)shadow & 255) == 0, "shadow buffer must be 256-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    const pv_vit_desc& d = p->d;
    PV_REQUIRE(w->conv_w && w->conv_b && w->W_pos && w->ln_final_w && w->ln_final_b, "missing global weights");
    if (d.use_cls_token) PV_REQUIRE(w->cls_token, "missing cls_token");
    if (d.layer_norm_pre) PV_REQUIRE(w->ln_pre_w && w->ln_pre_b, "missing ln_pre weights");
    if (d.has_head) PV_REQUIRE(w->W_H && w->b_H, "missing head weights");
    PV_REQUIRE(d.n_layers == 0 || w->layers, "missing layer weights");
    p->w = *w;
    unsigned char* cur = (unsigned char*)shadow;
    const int EB = p->EB, dm = d.d_model;
    {
        int rc;
        if ((rc = pack_block_and_head_shadows(p, w->layers, w->W_H, cur, stream))) return rc;
    }
    if (p->patch_prepack) {
        const int K = d.n_channels * d.patch_size * d.patch_size;
        if (p->Kp == K && pv_aligned16(w->conv_w)) {
            p->conv_wp = (unsigned char*)const_cast<void*>(w->conv_w);
        } else {
            p->conv_wp = cur;
            cur += seg((size_t)dm * p->Kp, EB);
            int rc;
            if ((rc = pv_launch_pad_rows_bf16(w->conv_w, p->conv_wp, dm, K, p->Kp, stream))) return rc;
        }
    }
    p->weights_set = true;
    return PV_OK;
}

namespace {
struct Workspace {
    size_t total;
    size_t embed, resid_a, resid_b, ln_out, q, k, v, z, resid_mid, mlp_post, lnf, head, pooled, patches;
};
Workspace carve(const pv_vit_plan* p, int B) {
    const pv_vit_desc& d = p->d;
    const size_t M = (size_t)B * p->T;
    const int EB = p->EB;
    Workspace w;
    size_t off = 0;
    auto take = [&](size_t elems) { size_t o = off; off += seg(elems, EB); return o; };
    w.embed = take((size_t)B * p->P * d.d_model);
    w.resid_a = take(M * d.d_model);
    w.resid_b = take(M * d.d_model);
    w.ln_out = take(M * d.d_model);
    w.q = take(M * p->HD);
    w.k = take(M * p->HD);
    w.v = take(M * p->HD);
    w.z = take(M * p->HD);
    w.resid_mid = take(M * d.d_model);
    w.mlp_post = take(M * d.d_mlp);
    w.lnf = take(M * d.d_model);
    w.head = take((size_t)B * (d.has_head ? d.n_classes : d.d_model * (d.pooling == PV_POOL_CLS_MEAN ? 2 : 1)));
    w.pooled = take((size_t)B * d.d_model);
    w.patches = p->patch_prepack ? take((size_t)B * p->P * p->Kp) : 0;
    w.total = off + 256;
    return w;
}
}  // namespace

extern "C" size_t pv_vit_workspace_bytes(const pv_vit_plan* p, int32_t batch) {
    if (!p || batch <= 0) return 0;
    return carve(p, batch).total;
}

// ---- the tapped forward ---------------------------------------------------------------------
namespace {
// One call runs one SEGMENT of the forward: from the model input, or from a residual stream resumed at position
// (first_block, entry_stage), to position (end_block, exit_stage), + the head.  Stages are PV_STAGE_* (positions inside a block: entry,
// ln1, q/k/v ready, scores, pattern, z ready, resid_mid, ln2, mlp pre, mlp post ready).  Every entry point fills one of these.
struct Segment {
    const void* images;        // vision plan: exactly one of images / resid_in
    const int64_t* tokens;     // text plan (pv_text_forward alone passes them)
    const void* resid_in;      // the residual stream the rest of block first_block adds to: resid_pre up to PV_STAGE_Z, resid_mid behind
    const void* act_in[3];     // the (hook-edited) activations of entry_stage: ln normalized fp32 | q, k, v | scores, v | pattern, v | z | mlp pre | mlp post
    int32_t B, first_block, entry_stage, end_block, exit_stage, run_head, n_taps;
    const pv_tap* taps;
    void *workspace, *out;
    size_t workspace_bytes;
    hipStream_t stream;
};
Segment segment_io(int32_t B, int32_t run_head, const pv_tap* taps, int32_t n_taps, void* workspace, size_t workspace_bytes, void* out, void* stream) {
    Segment s = {};
    s.B = B; s.run_head = run_head; s.taps = taps; s.n_taps = n_taps;
    s.workspace = workspace; s.workspace_bytes = workspace_bytes; s.out = out; s.stream = (hipStream_t)stream;
    return s;
}

// Every rule of a call, before any launch; carves the workspace on the way.  (split_plan.py's EXIT table states the act_in rows.)
int check_segment(const pv_vit_plan* p, const Segment& s, Workspace& ws) {
    PV_REQUIRE(p && s.workspace, "null argument");
    const int32_t n_layers = p->d.n_layers, first_block = s.first_block, end_block = s.end_block, entry_stage = s.entry_stage,
                  exit_stage = s.exit_stage, run_head = s.run_head;
    const void* const* act_in = s.act_in;
    PV_REQUIRE(s.tokens || ((s.images != nullptr) != (s.resid_in != nullptr)), "exactly one of images / resid_in");
    PV_REQUIRE(!s.resid_in || pv_aligned16(s.resid_in), "resid_in must be 16-byte aligned");
    PV_REQUIRE(entry_stage >= 0 && entry_stage <= PV_STAGE_MLP_POST && exit_stage >= 0 && exit_stage <= PV_STAGE_MLP_POST, "stage");
    PV_REQUIRE(s.resid_in ? (first_block >= 0 && first_block <= n_layers) : (first_block == 0 && !entry_stage), "segment start");
    PV_REQUIRE(first_block <= end_block && end_block <= n_layers, "segment end (n_blocks out of range)");
    PV_REQUIRE(!entry_stage || first_block < n_layers, "a mid-block entry needs a block to resume");
    PV_REQUIRE(!exit_stage || (end_block < n_layers && !run_head), "a mid-block exit stops inside block end_block");
    PV_REQUIRE(first_block < end_block || entry_stage < exit_stage || (first_block == end_block && !exit_stage && !entry_stage),
               "empty or backward segment");
    if (entry_stage == PV_STAGE_QKV) PV_REQUIRE(act_in[0] && act_in[1] && act_in[2], "entry at PV_STAGE_QKV needs q, k, v");
    if (entry_stage == PV_STAGE_Z || entry_stage == PV_STAGE_MLP_POST || entry_stage == PV_STAGE_LN1 || entry_stage == PV_STAGE_LN2 ||
        entry_stage == PV_STAGE_MLP_PRE)
        PV_REQUIRE(act_in[0], "entry at PV_STAGE_LN1 / Z / LN2 / MLP_PRE / MLP_POST needs the activation");
    if (entry_stage == PV_STAGE_SCORES || entry_stage == PV_STAGE_PATTERN)
        PV_REQUIRE(act_in[0] && act_in[1], "entry at PV_STAGE_SCORES / PV_STAGE_PATTERN needs the activation and v");
    for (int i = 0; i < 3; ++i) PV_REQUIRE(!act_in[i] || pv_aligned16(act_in[i]), "activation inputs must be 16-byte aligned");
    PV_REQUIRE(!s.tokens || p->is_text, "pv_text_forward needs a plan of pv_text_plan_create (a vision plan runs through pv_vit_forward*)");
    PV_REQUIRE(s.tokens || !p->is_text, "a text plan runs through pv_text_forward, a vision plan through pv_vit_forward*");
    PV_REQUIRE(p->weights_set, "pv_vit_plan_set_weights has not been called");
    PV_REQUIRE(s.B > 0, "batch must be positive");
    PV_REQUIRE(!run_head || end_block == n_layers, "run_head requires all blocks");
    PV_REQUIRE(!run_head || s.out, "run_head requires an output buffer");
    PV_REQUIRE(((uintptr_t)s.workspace & 255) == 0, "workspace must be 256-byte aligned");
    PV_REQUIRE(!s.images || pv_aligned16(s.images), "images must be 16-byte aligned");
    ws = carve(p, s.B);
    PV_REQUIRE(s.workspace_bytes >= ws.total, "workspace too small");
    return PV_OK;
}

// What the steps of one call share.
struct Fwd {
    const pv_vit_plan* p;
    const pv_vit_desc& d;
    const Segment& s;
    const void* const* act_in;
    const int dt, B, T, M;
    const bool bf16;
    const hipStream_t stream;
    unsigned char* const wsb;
    const Workspace ws;
    std::vector<void*> tap;     // [layer][slot]: where a tapped buffer goes, nullptr = not tapped
    bool resid_in_a = true;     // which workspace residual buffer may hold the residual stream
    Fwd(const pv_vit_plan* p, const Segment& s, const Workspace& ws)
        : p(p), d(p->d), s(s), act_in(s.act_in), dt(p->d.dtype), B(s.B), T(p->T), M(s.B * p->T), bf16(p->d.dtype == PV_DTYPE_BF16),
          stream(s.stream), wsb((unsigned char*)s.workspace), ws(ws), tap((size_t)PV_SLOT__COUNT * (size_t)(p->d.n_layers + 1), nullptr) {}
    void*& tap_at(int slot, int layer) { return tap[(size_t)layer * PV_SLOT__COUNT + slot]; }
    // the tap's destination when the slot is tapped, else its workspace buffer
    void* pick(int slot, int layer, size_t ws_off) { return tap_at(slot, layer) ? tap_at(slot, layer) : (void*)(wsb + ws_off); }
    int set_taps(const pv_tap* taps, int n_taps) {
        for (int i = 0; i < n_taps; ++i) {
            const pv_tap& t = taps[i];
            PV_REQUIRE(t.slot >= 0 && t.slot < PV_SLOT__COUNT && t.dst, "bad tap slot");
            const int layer = t.slot >= PV_SLOT_LN1_SCALE ? t.layer : 0;
            PV_REQUIRE(layer >= 0 && layer < d.n_layers + 1, "bad tap layer");
            PV_REQUIRE(pv_aligned16(t.dst), "tap destinations must be 16-byte aligned");
            PV_REQUIRE(bf16 || (t.slot != PV_SLOT_LNPRE_NORM_F32 && t.slot != PV_SLOT_LNF_NORM_F32 &&
                                t.slot != PV_SLOT_LN1_NORM_F32 && t.slot != PV_SLOT_LN2_NORM_F32),
                       "*_NORM_F32 slots exist only in bf16 mode");
            PV_REQUIRE(!p->is_text || (t.slot != PV_SLOT_LNPRE_SCALE && t.slot != PV_SLOT_LNPRE_NORM_F32 && t.slot != PV_SLOT_LNPRE_OUT),
                       "a text plan has no PV_SLOT_LNPRE_* slots: ln_pre never runs (base_text_transformer.py:139-146)");
            tap_at(t.slot, layer) = t.dst;
        }
        return PV_OK;
    }
};

// what the six linear layers' GEMMs share; the call sites set the epilogue's operands (and the patch gather's A mode)
GemmParams linear(const void* A, int64_t lda, const void* Bt, int64_t ldb, int M, int N, int K, int epi) {
    GemmParams g = {};
    g.A = A; g.lda = lda; g.a_mode = PV_A_PLAIN; g.Bt = Bt; g.ldb = ldb; g.M = M; g.N = N; g.K = K; g.epi = epi;
    return g;
}

// ---- patch embedding: stride-p conv as an im2col-free GEMM (patch_embedding.py:26-32), then cls + pos (+ ln_pre) (base_vit.py:171-185)
int embed_vision(Fwd& F, void*& resid) {
    const pv_vit_plan* p = F.p;
    const pv_vit_desc& d = F.d;
    const void* images = F.s.images;
    const int dm = d.d_model, K = d.n_channels * d.patch_size * d.patch_size;
    void* embed = F.pick(PV_SLOT_EMBED, 0, F.ws.embed);
    GemmParams g;
    int rc;
    if (p->patch_prepack && ((uintptr_t)images & 3) == 0) {
        void* rows = F.wsb + F.ws.patches;
        if ((rc = pv_launch_patch_pack_bf16(images, rows, F.B, d.n_channels, d.image_size, d.patch_size, p->G, p->Kp, F.stream))) return rc;
        g = linear(rows, p->Kp, p->conv_wp, p->Kp, F.B * p->P, dm, p->Kp, PV_EPI_BIAS);
    } else {
        g = linear(images, 0, p->w.conv_w, K, F.B * p->P, dm, K, PV_EPI_BIAS);
        g.a_mode = PV_A_PATCH; g.pC = d.n_channels; g.pP = d.patch_size; g.pS = d.image_size; g.pG = p->G;
    }
    g.bias0 = p->w.conv_b; g.out0 = embed; g.ldo = dm;
    if ((rc = pv_launch_gemm(F.dt, g, F.stream))) return rc;
    LnParams L = {};
    L.x = embed; L.rows = F.M; L.d = dm; L.eps = d.eps; L.embed = 1; L.T = F.T; L.use_cls = d.use_cls_token ? 1 : 0;
    L.cls = p->w.cls_token; L.pos = p->w.W_pos;
    if (d.layer_norm_pre) {
        L.do_ln = 1; L.w = p->w.ln_pre_w; L.b = p->w.ln_pre_b;
        L.full_out = F.tap_at(PV_SLOT_FULL_EMBED, 0);
        L.scale_out = (float*)F.tap_at(PV_SLOT_LNPRE_SCALE, 0);
        L.norm_f32_out = (float*)F.tap_at(PV_SLOT_LNPRE_NORM_F32, 0);
        resid = F.pick(PV_SLOT_LNPRE_OUT, 0, F.ws.resid_a);
        L.out = resid;
    } else {
        L.do_ln = 0;
        resid = F.pick(PV_SLOT_FULL_EMBED, 0, F.ws.resid_a);
        L.full_out = resid;
    }
    return pv_launch_ln(F.dt, L, F.stream);
}

// ---- token + position embedding (base_text_transformer.py:125-143): hook_embed is the gather itself, hook_full_embed the residual
// stream entering block 0
int embed_text(Fwd& F, void*& resid) {
    resid = F.pick(PV_SLOT_FULL_EMBED, 0, F.ws.resid_a);
    return pv_launch_token_embed(F.dt, F.s.tokens, F.p->token_embed, F.p->pos_embed, F.tap_at(PV_SLOT_EMBED, 0), resid, F.B, F.T,
                                 F.d.d_model, F.p->vocab, F.stream);
}

// ---- the block's steps (transformer_block.py:80-138) -----------------------------------------
// ln1 (transformer_block.py:106-109) and ln2 (:130) (layer_norm.py:75-93); scale_slot: PV_SLOT_LN1_SCALE | PV_SLOT_LN2_SCALE.  Both share
// ln_out.  hooked: behind a hooked .hook_scale / .hook_normalized the (edited) fp32 normalized tensor act_in[0] is rounded to the storage
// dtype like the module's own last step (layer_norm.py:93) -- into the workspace, never into a tap
int block_ln(Fwd& F, int l, int scale_slot, const void* w, const void* b, const void* x, bool hooked, void*& out) {
    static_assert(PV_SLOT_LN1_NORM_F32 == PV_SLOT_LN1_SCALE + 1 && PV_SLOT_LN1_OUT == PV_SLOT_LN1_SCALE + 2 &&
                  PV_SLOT_LN2_NORM_F32 == PV_SLOT_LN2_SCALE + 1 && PV_SLOT_LN2_OUT == PV_SLOT_LN2_SCALE + 2, "a LayerNorm's three slots");
    const int dm = F.d.d_model;
    if (hooked) {
        out = F.bf16 ? (void*)(F.wsb + F.ws.ln_out) : const_cast<void*>(F.act_in[0]);
        return F.bf16 ? pv_launch_cast_from_f32(F.dt, (const float*)F.act_in[0], out, (int64_t)F.M * dm, F.stream) : PV_OK;
    }
    out = F.pick(scale_slot + 2, l, F.ws.ln_out);
    LnParams L = {};
    L.x = x; L.ldx = dm; L.rows = F.M; L.d = dm; L.eps = F.d.eps; L.do_ln = 1;
    L.w = w; L.b = b;
    L.scale_out = (float*)F.tap_at(scale_slot, l);
    L.norm_f32_out = (float*)F.tap_at(scale_slot + 1, l);
    L.out = out;
    return pv_launch_ln(F.dt, L, F.stream);
}

// q, k, v (attention.py:186-244) as one GEMM against the packed [3*H*dh][d] shadow
int block_qkv(Fwd& F, int l, const void* ln1, void*& q, void*& k, void*& v) {
    const pv_vit_layer_weights& W = F.p->lw[l];
    const int dm = F.d.d_model, HD = F.p->HD;
    q = F.pick(PV_SLOT_Q, l, F.ws.q);
    k = F.pick(PV_SLOT_K, l, F.ws.k);
    v = F.pick(PV_SLOT_V, l, F.ws.v);
    GemmParams g = linear(ln1, dm, F.p->sh[l].Wqkv, dm, F.M, 3 * HD, dm, PV_EPI_QKV);
    g.nsplit = HD;
    g.bias0 = W.b_Q; g.bias1 = W.b_K; g.bias2 = W.b_V; g.out0 = q; g.out1 = k; g.out2 = v; g.ldo = HD;
    return pv_launch_gemm(F.dt, g, F.stream);
}

// scores / pattern / z (attention.py:135-152, 246-281): the whole core from q, k, v (es < PV_STAGE_SCORES) -- or, behind a hooked
// hook_attn_scores / hook_pattern (es = that stage), the rest of it from the edited tensor act_in[0] and v = act_in[1]
int block_attention(Fwd& F, int l, int es, const void* q, const void* k, const void* v, void*& z) {
    z = F.pick(PV_SLOT_Z, l, F.ws.z);
    AttnParams a = {};
    a.z = z;
    a.B = F.B; a.T = F.T; a.H = F.d.n_heads; a.dh = F.d.d_head; a.attn_scale = F.d.attn_scale;
    if (es < PV_STAGE_SCORES) {
        a.q = q; a.k = k; a.v = v;
        a.scores = F.tap_at(PV_SLOT_SCORES, l); a.pattern = F.tap_at(PV_SLOT_PATTERN, l);
        a.causal = F.p->causal;
        return pv_launch_attention(F.dt, a, F.stream);
    }
    a.v = F.act_in[1];
    if (es == PV_STAGE_SCORES) { a.scores = const_cast<void*>(F.act_in[0]); a.pattern = F.tap_at(PV_SLOT_PATTERN, l); }
    else a.pattern = const_cast<void*>(F.act_in[0]);
    return pv_launch_attention_resume(F.dt, a, es == PV_STAGE_SCORES ? 1 : 0, F.stream);
}

// attn_out = z W_O + b_O ; resid_mid = resid_pre + attn_out (attention.py:155-167 ; block :117-124)
int block_oproj(Fwd& F, int l, const void* z, const void* resid_pre, void*& resid_mid) {
    const int dm = F.d.d_model, HD = F.p->HD;
    resid_mid = F.pick(PV_SLOT_RESID_MID, l, F.ws.resid_mid);
    GemmParams g = linear(z, HD, F.p->sh[l].WoT, HD, F.M, dm, HD, PV_EPI_RESID);
    g.bias0 = F.p->lw[l].b_O;
    g.out0 = F.tap_at(PV_SLOT_ATTN_OUT, l); g.out1 = resid_mid; g.ldo = dm; g.resid = resid_pre; g.ldr = dm;
    return pv_launch_gemm(F.dt, g, F.stream);
}

// mlp (mlp.py:65-80): pre -> act -> post as one GEMM -- or, behind a hooked mlp.hook_pre (pre_hooked), the activation function alone
// on the edited pre-activation act_in[0] (mlp.py:67-72)
int block_mlp_in(Fwd& F, int l, bool pre_hooked, const void* ln2, void*& post) {
    const int dm = F.d.d_model, dmlp = F.d.d_mlp;
    post = F.pick(PV_SLOT_MLP_POST, l, F.ws.mlp_post);
    if (pre_hooked) return pv_launch_act(F.dt, F.d.activation, F.act_in[0], post, (int64_t)F.M * dmlp, F.stream);
    GemmParams g = linear(ln2, dm, F.p->sh[l].WinT, dm, F.M, dmlp, dm, PV_EPI_ACT);
    g.act = F.d.activation; g.bias0 = F.p->lw[l].b_in;
    g.out0 = F.tap_at(PV_SLOT_MLP_PRE, l); g.out1 = post; g.ldo = dmlp;
    return pv_launch_gemm(F.dt, g, F.stream);
}

// mlp_out ; resid_post = resid_mid + mlp_out (block :131-134), which becomes the residual stream
int block_mlp_out(Fwd& F, int l, const void* post, const void* resid_mid, void*& resid) {
    const int dm = F.d.d_model, dmlp = F.d.d_mlp;
    void* resid_post = F.tap_at(PV_SLOT_RESID_POST, l);
    if (!resid_post) {
        // the workspace buffer NOT holding resid_pre (resid_pre is dead after the O-proj, but keep it simple and safe: ping-pong)
        resid_post = F.wsb + (F.resid_in_a ? F.ws.resid_b : F.ws.resid_a);
        F.resid_in_a = !F.resid_in_a;
    }
    GemmParams g = linear(post, dmlp, F.p->sh[l].WoutT, dmlp, F.M, dm, dmlp, PV_EPI_RESID);
    g.bias0 = F.p->lw[l].b_out;
    g.out0 = F.tap_at(PV_SLOT_MLP_OUT, l); g.out1 = resid_post; g.ldo = dm; g.resid = resid_mid; g.ldr = dm;
    resid = resid_post;
    return pv_launch_gemm(F.dt, g, F.stream);
}

// Block l of a segment, stage by stage in PV_STAGE_* order.  es: the stage the block is entered at (PV_STAGE_ENTRY: its start): a stage
// before es is skipped, the one AT es adopts the caller's act_in, every later one is computed here.  xs: the stage the segment stops
// at inside this block (PV_STAGE_ENTRY: it runs through).  `resid` is the residual stream the rest of the block adds to -- resid_pre,
// or resid_mid when es >= PV_STAGE_MID -- and leaves as resid_post (an exit at PV_STAGE_MID: as resid_mid; any other exit: unchanged).
int run_block(Fwd& F, int l, int es, int xs, void*& resid) {
    const pv_vit_layer_weights& W = F.p->lw[l];
    void *ln1 = nullptr, *q = nullptr, *k = nullptr, *v = nullptr, *z = nullptr, *resid_mid = nullptr, *ln2 = nullptr, *post = nullptr;
    int rc = PV_OK;
    if (es <= PV_STAGE_LN1) rc = block_ln(F, l, PV_SLOT_LN1_SCALE, W.ln1_w, W.ln1_b, resid, es == PV_STAGE_LN1, ln1);
    if (rc || xs == PV_STAGE_LN1) return rc;

    if (es < PV_STAGE_QKV) rc = block_qkv(F, l, ln1, q, k, v);
    else if (es == PV_STAGE_QKV) { q = const_cast<void*>(F.act_in[0]); k = const_cast<void*>(F.act_in[1]); v = const_cast<void*>(F.act_in[2]); }
    if (rc || xs == PV_STAGE_QKV) return rc;

    // scores, pattern and z are one kernel: an exit at any of the three runs the whole core first
    if (es <= PV_STAGE_PATTERN) rc = block_attention(F, l, es, q, k, v, z);
    else if (es == PV_STAGE_Z) z = const_cast<void*>(F.act_in[0]);
    if (rc || xs == PV_STAGE_SCORES || xs == PV_STAGE_PATTERN || xs == PV_STAGE_Z) return rc;

    if (es < PV_STAGE_MID) rc = block_oproj(F, l, z, resid, resid_mid);
    else resid_mid = resid;
    if (xs == PV_STAGE_MID) resid = resid_mid;
    if (rc || xs == PV_STAGE_MID) return rc;

    if (es <= PV_STAGE_LN2) rc = block_ln(F, l, PV_SLOT_LN2_SCALE, W.ln2_w, W.ln2_b, resid_mid, es == PV_STAGE_LN2, ln2);
    if (rc || xs == PV_STAGE_LN2) return rc;

    // mlp pre and post are one GEMM
    if (es <= PV_STAGE_MLP_PRE) rc = block_mlp_in(F, l, es == PV_STAGE_MLP_PRE, ln2, post);
    else post = const_cast<void*>(F.act_in[0]);
    if (rc || xs == PV_STAGE_MLP_PRE || xs == PV_STAGE_MLP_POST) return rc;

    return block_mlp_out(F, l, post, resid_mid, resid);
}

// ---- ln_final on all tokens only if one of its taps is requested or the pooling reads them all (lnf_all), else on the CLS rows only
// (a text plan: on the EOT rows only).  lnf_ld: the row stride (elements) between the pooled rows of consecutive images
int head_ln_final(Fwd& F, const void* resid, bool lnf_all, void*& lnf, int64_t& lnf_ld) {
    const int dm = F.d.d_model;
    lnf = F.pick(PV_SLOT_LNF_OUT, 0, F.ws.lnf);
    LnParams L = {};
    L.x = resid; L.d = dm; L.eps = F.d.eps; L.do_ln = 1; L.w = F.p->w.ln_final_w; L.b = F.p->w.ln_final_b; L.out = lnf;
    lnf_ld = lnf_all ? (int64_t)F.T * dm : dm;
    if (lnf_all) {
        L.ldx = dm; L.rows = F.M;
        L.scale_out = (float*)F.tap_at(PV_SLOT_LNF_SCALE, 0);
        L.norm_f32_out = (float*)F.tap_at(PV_SLOT_LNF_NORM_F32, 0);
    } else if (F.p->is_text) {
        // the residual rows at the EOT tokens first (base_text_transformer.py:151), LayerNorm on those B rows
        void* rows = F.wsb + F.ws.pooled;
        int rc;
        if ((rc = pv_launch_eot_rows(F.dt, F.s.tokens, resid, rows, F.B, F.T, dm, F.stream))) return rc;
        L.x = rows; L.ldx = dm; L.rows = F.B;
    } else {
        L.ldx = (int64_t)F.T * dm; L.rows = F.B;
    }
    return pv_launch_ln(F.dt, L, F.stream);
}

// ---- ln_final -> pooled row (base_vit.py:195-208) -> head (head.py:27-37) -> hook_post_head_pre_normalize -> F.normalize
int head(Fwd& F, const void* resid) {
    const pv_vit_plan* p = F.p;
    const pv_vit_desc& d = F.d;
    const int dm = d.d_model, B = F.B, T = F.T, dt = F.dt;
    void* const out = F.s.out;
    const bool lnf_all = d.pooling != PV_POOL_CLS || F.tap_at(PV_SLOT_LNF_SCALE, 0) || F.tap_at(PV_SLOT_LNF_NORM_F32, 0) || F.tap_at(PV_SLOT_LNF_OUT, 0);
    void* lnf;
    int64_t lnf_ld;
    int rc;
    if ((rc = head_ln_final(F, resid, lnf_all, lnf, lnf_ld))) return rc;
    const bool cls_mean = d.pooling == PV_POOL_CLS_MEAN;
    const int nout = d.has_head ? d.n_classes : (cls_mean ? 2 * dm : dm);
    void* head_tap = F.tap_at(PV_SLOT_HEAD_OUT, 0);
    void* hb = head_tap ? head_tap : (d.normalize_output ? (void*)(F.wsb + F.ws.head) : out);
    if (p->is_text && lnf_all) {
        // x[arange(B), tokens.argmax(dim=-1)] of the ln_final output (base_text_transformer.py:151)
        void* pooled = F.wsb + F.ws.pooled;
        if ((rc = pv_launch_eot_rows(dt, F.s.tokens, lnf, pooled, B, T, dm, F.stream))) return rc;
        lnf = pooled;
        lnf_ld = dm;
    }
    if (d.pooling != PV_POOL_CLS) {
        // "gaap": the mean over all tokens feeds the head (or IS the output); dino-vitb: [B, d, 2] = (cls, mean over the patches)
        void* pooled = (d.has_head) ? (void*)(F.wsb + F.ws.pooled) : hb;
        if ((rc = pv_launch_token_mean(dt, lnf, pooled, B, T, dm, cls_mean ? 1 : 0, cls_mean ? 1 : 0, F.stream))) return rc;
        lnf = pooled;
        lnf_ld = dm;
    }
    if (d.has_head) {
        GemmParams g = linear(lnf, lnf_ld, p->WhT, dm, B, nout, dm, PV_EPI_BIAS);
        g.bias0 = p->w.b_H; g.out0 = hb; g.ldo = nout;
        if ((rc = pv_launch_gemm(dt, g, F.stream))) return rc;
    } else if (d.pooling == PV_POOL_CLS) {
        PV_HIP_CHECK(hipMemcpy2DAsync(hb, (size_t)dm * p->EB, lnf, (size_t)lnf_ld * p->EB, (size_t)dm * p->EB, B,
                                      hipMemcpyDeviceToDevice, F.stream));
    }
    if (d.normalize_output) {
        // dim = -1 of [B, d, 2] is the (cls, mean) pair of one channel (base_vit.py:214-215 on the concatenated tensor)
        return cls_mean ? pv_launch_l2norm(dt, hb, out, B * dm, 2, F.stream) : pv_launch_l2norm(dt, hb, out, B, nout, F.stream);
    }
    if (hb != out) PV_HIP_CHECK(hipMemcpyAsync(out, hb, (size_t)B * nout * p->EB, hipMemcpyDeviceToDevice, F.stream));
    return PV_OK;
}

// validate -> context -> embed (or adopt resid_in: a resumed forward skips the embedding) -> blocks -> head
int run_segment(const pv_vit_plan* p, const Segment& s) {
    Workspace ws;
    int rc;
    if ((rc = check_segment(p, s, ws))) return rc;
    Fwd F(p, s, ws);
    if ((rc = F.set_taps(s.taps, s.n_taps))) return rc;
    void* resid = const_cast<void*>(s.resid_in);
    if (!resid && (rc = p->is_text ? embed_text(F, resid) : embed_vision(F, resid))) return rc;
    // blocks [first_block, end_block) in full; with exit_stage also block end_block up to it; with entry_stage the first block resumes behind it
    const int last_block = s.exit_stage ? s.end_block + 1 : s.end_block;
    for (int l = s.first_block; l < last_block; ++l)
        if ((rc = run_block(F, l, l == s.first_block ? s.entry_stage : PV_STAGE_ENTRY, l == s.end_block ? s.exit_stage : PV_STAGE_ENTRY, resid))) return rc;
    return s.run_head ? head(F, resid) : PV_OK;
}
}  // namespace

extern "C" int pv_vit_forward(pv_vit_plan* p, const void* images, int32_t B, int32_t n_blocks, int32_t run_head, const pv_tap* taps,
                              int32_t n_taps, void* workspace, size_t workspace_bytes, void* out, void* stream) {
    PV_REQUIRE(images, "null argument");
    Segment s = segment_io(B, run_head, taps, n_taps, workspace, workspace_bytes, out, stream);
    s.images = images; s.end_block = n_blocks;
    return run_segment(p, s);
}

extern "C" int pv_vit_forward_stage(pv_vit_plan* p, const void* images, const void* resid_in, const void* act_in0, const void* act_in1,
                                    const void* act_in2, int32_t B, int32_t first_block, int32_t entry_stage, int32_t end_block,
                                    int32_t exit_stage, int32_t run_head, const pv_tap* taps, int32_t n_taps, void* workspace,
                                    size_t workspace_bytes, void* out, void* stream) {
    Segment s = segment_io(B, run_head, taps, n_taps, workspace, workspace_bytes, out, stream);
    s.images = images; s.resid_in = resid_in;
    s.act_in[0] = act_in0; s.act_in[1] = act_in1; s.act_in[2] = act_in2;
    s.first_block = first_block; s.entry_stage = entry_stage; s.end_block = end_block; s.exit_stage = exit_stage;
    return run_segment(p, s);
}

extern "C" int pv_text_forward(pv_vit_plan* p, const int64_t* tokens, int32_t B, int32_t run_head, const pv_tap* taps, int32_t n_taps,
                               void* workspace, size_t workspace_bytes, void* out, void* stream) {
    PV_REQUIRE(p && tokens, "null argument");
    Segment s = segment_io(B, run_head, taps, n_taps, workspace, workspace_bytes, out, stream);
    s.tokens = tokens; s.end_block = p->d.n_layers;
    return run_segment(p, s);
}

// ---- kernel-level entry points -------------------------------------------------------------
extern "C" int pv_attention(int32_t dtype, const void* q, const void* k, const void* v, int32_t B, int32_t T, int32_t H, int32_t dh,
                            float attn_scale, int32_t causal, void* scores, void* pattern, void* z, void* stream) {
    PV_REQUIRE(B > 0 && T > 0 && H > 0 && dh > 0, "pv_attention: dims");
    AttnParams a = {};
    a.q = q; a.k = k; a.v = v; a.z = z; a.scores = scores; a.pattern = pattern;
    a.B = B; a.T = T; a.H = H; a.dh = dh; a.attn_scale = attn_scale; a.causal = causal ? 1 : 0;
    return pv_launch_attention(dtype, a, (hipStream_t)stream);
}
extern "C" int pv_gemm_bias(int32_t dtype, const void* A, int64_t lda, const void* Bt, int64_t ldb,
                            const void* bias, void* C, int64_t ldc, int32_t M, int32_t N, int32_t K,
                            void* stream) {
    GemmParams g = {};
    g.A = A; g.lda = lda; g.a_mode = PV_A_PLAIN; g.Bt = Bt; g.ldb = ldb; g.M = M; g.N = N; g.K = K;
    g.epi = PV_EPI_BIAS; g.bias0 = bias; g.out0 = C; g.ldo = ldc;
    return pv_launch_gemm(dtype, g, (hipStream_t)stream);
}

extern "C" int pv_gemm_epilogue(int32_t dtype, int32_t epi, int32_t act, const void* A, int64_t lda, const void* Bt, int64_t ldb,
                                const void* bias, const void* resid, int64_t ldr, void* out0, void* out1, int64_t ldo,
                                int32_t M, int32_t N, int32_t K, void* stream) {
    PV_REQUIRE(epi == PV_GEMM_EPI_BIAS || epi == PV_GEMM_EPI_RESID || epi == PV_GEMM_EPI_ACT, "pv_gemm_epilogue: epi");
    GemmParams g = {};
    g.A = A; g.lda = lda; g.a_mode = PV_A_PLAIN; g.Bt = Bt; g.ldb = ldb; g.M = M; g.N = N; g.K = K;
    g.epi = epi; g.act = act; g.bias0 = bias; g.out0 = out0; g.out1 = out1; g.ldo = ldo; g.resid = resid; g.ldr = ldr;
    return pv_launch_gemm(dtype, g, (hipStream_t)stream);
}

extern "C" int pv_transpose_batched(int32_t elem_bytes, const void* in, void* out, int32_t batch,
                                    int32_t R, int32_t C, void* stream) {
    PV_REQUIRE(in && out, "null argument");
    return pv_launch_transpose(elem_bytes, in, out, batch, R, C, (hipStream_t)stream);
}
