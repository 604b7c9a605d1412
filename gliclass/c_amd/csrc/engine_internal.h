// What engine.hip (load, workspace, forwards) and engine_debug.hip (developer entries that allocate their own buffers or launch kernels
// outside a forward) share: the engine itself, the error setter behind glc_last_error() and the two check macros.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/gliclass_hip.h"
#include "glc_kernels.h"

void glc_set_err(const std::string& s);      // engine.hip: the calling thread's glc_last_error() text

#define HIPCHK(expr, ret)                                                                          \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            glc_set_err(std::string(#expr) + ": " + hipGetErrorString(_e));                        \
            return ret;                                                                            \
        }                                                                                          \
    } while (0)
#define KCHK(expr, ret)                                                                            \
    do {                                                                                           \
        const char* _m = (expr);                                                                   \
        if (_m) { glc_set_err(_m); return ret; }                                                   \
    } while (0)

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
inline size_t esize(int dtype) { return dtype == GLC_F32 ? 4 : 2; }

enum { PC_SCAN = 0, PC_EMBED, PC_QKV, PC_ATTN, PC_ATTN_OUT, PC_LN, PC_FFN1, PC_FFN2, PC_HEAD, PC_LAST, PC_N };
const char* const kProfNames[PC_N] = {"scan_rows", "embed_ln", "gemm_qkv", "attention", "gemm_attn_out", "layernorm",
                                      "gemm_ffn1_gelu", "gemm_ffn2", "head", "last_layer_pruned"};

struct DecLayerW {                     // decoder-style backbone (decoder.hip)
    void *Wqkv = nullptr, *Wo = nullptr, *Wgu = nullptr, *Wd = nullptr;       // T: [(nq+2nkv)d, H], [H, nq d], [2I, H] (gate rows | up rows), [H, I]
    float *bqkv = nullptr, *ln1 = nullptr, *ln2 = nullptr;                    // f32 (bqkv: null without attn_bias — Llama, Qwen3)
    void *Wqkvf = nullptr, *Wguf = nullptr;                                   // fp32 mode, RMSNorm folded into the GEMMs: Wqkv diag(ln1), Wgu diag(ln2), group-split
    void *Wqkvf_x = nullptr, *Wo_x = nullptr, *Wguf_x = nullptr, *Wd_x = nullptr;   // MX pipeline: the same four as GX rows + their fp8 exponents
    int ws_qkvf = 0, ws_o = 0, ws_guf = 0, ws_d = 0;
    void *Wqkv_x = nullptr, *Wgu_x = nullptr;                                 // ModernBERT's MX pipeline (no norm fold): Wqkv and Wi as GX rows (Wo_x, Wd_x above)
    int ws_qkv = 0, ws_gu = 0;
    float* bqkv_p = nullptr;            // bqkv in the row order of a Wqkvf_x built for the RoPE epilogue (glc_rope_perm128), else null
    bool qkv_perm = false;              // Wqkvf_x's rows are in that order (with or without a bias to go with them)
    float *qn = nullptr, *kn = nullptr; // qk_norm (Qwen3): the gains [head_dim] of self_attn.q_norm / k_norm, f32; else null
};

struct LayerW {
    void *Wqkv = nullptr, *Wo = nullptr, *W1 = nullptr, *W2 = nullptr;       // T
    float *bqkv = nullptr, *bo = nullptr, *b1 = nullptr, *b2 = nullptr;       // f32
    float *ln1g = nullptr, *ln1b = nullptr, *ln2g = nullptr, *ln2b = nullptr; // f32
    void *PK = nullptr, *PQ = nullptr;                                        // T [nh, P, 64]
    void *PKs = nullptr, *PQs = nullptr;                                      // fp32 mode: the same tables as split-f16 units (band kernel, AttnArgs::split)
    // LayerNorm folded into the group-split GEMMs (GemmArgs::a_stats): W1 . diag(ln1 gamma), Wqkv . diag(previous layer's ln2 gamma)
    // as group-split rows, their row sums c and the folded biases d = W beta + b
    void *W1f = nullptr, *Wqkvf = nullptr;
    float *c1 = nullptr, *d1 = nullptr, *cq = nullptr, *dq = nullptr;
    // MX pipeline (glc_engine::mx): the projection weights once more as GX rows (glc_common.h) with their fp8 exponents
    void *PKm = nullptr, *PQm = nullptr;                                     // the position tables as MX tiles (attention_mx.hip)
    void *Wqkv_x = nullptr, *Wqkvf_x = nullptr, *Wo_x = nullptr, *W1f_x = nullptr, *W2_x = nullptr;
    int ws_qkv = 0, ws_qkvf = 0, ws_o = 0, ws_1f = 0, ws_2 = 0;
};

// Captured-graph replay (glc_engine_set_graph_replay): what a cached forward is filed under — everything that decides which kernels a forward
// launches or what arguments they get — and what it leaves behind for the glc_debug_last_forward_* queries
struct GraphKey {
    int backbone, head, B, S, Sp, C;      // head: the head kind (constant per engine; kept in the key so that the key alone names the captured launch sequence)
    int gs_mode, mx, mx_attn, ln_fused, prune, attn_impl, prec_mask, act_sc, sticky, full_lines, mx_small;
    unsigned long long ws_gen;
    const void *ids, *mask, *logits;
    bool operator==(const GraphKey& o) const {
        return backbone == o.backbone && head == o.head && B == o.B && S == o.S && Sp == o.Sp && C == o.C && gs_mode == o.gs_mode && mx == o.mx && mx_attn == o.mx_attn &&
               ln_fused == o.ln_fused && prune == o.prune && attn_impl == o.attn_impl && prec_mask == o.prec_mask && act_sc == o.act_sc &&
               sticky == o.sticky && full_lines == o.full_lines && mx_small == o.mx_small && ws_gen == o.ws_gen && ids == o.ids && mask == o.mask && logits == o.logits;
    }
};
struct GraphEntry {
    GraphKey key;
    hipGraphExec_t exec = nullptr;      // null: the key has run eagerly once (workspace sized, tables and MX weights built, LDS limits raised)
    bool ineligible = false;            // its capture failed: eager from now on
    unsigned long long tick = 0;        // last use (least recently used goes first)
    bool gs = false, lnf = false, mx = false, mx_attn = false, rope_epi = false, pruned = false;      // the forward's last_* answers
    int mx128 = 0;
};
constexpr int kGraphCacheMax = 16;      // graph executables per engine
constexpr int kGraphKeysMax = 64;       // ... and keys remembered in all (warmed-up or ineligible ones included)

struct glc_engine {
    glc_model_config cfg{};
    int dtype = GLC_F32, device = 0, attn_impl = 0;
    bool prune_last = true;         // last layer only on the rows the head reads (exact; every backbone, not with average pooling or keep_hidden)
    bool last_pruned = false;       // the last forward ran that compact last layer
    bool w_presplit = false;        // weights of the split-f16 fp32 GEMMs are split once at load (encoder layers in fp32 mode; head projectors in every mode)
    bool dec_split = false;         // decoder backbone, fp32 mode: RoPE/layout pass writes split-f16 units, grouped-query attention on three-MFMA products
    bool attn_split = false;        // fp32 mode: band attention on split-f16 operands (three f16 MFMAs per product); GLICLASS_F32_ATTN=native turns it off
    bool mx_built = false, mx = false;   // MX cross-term projections (gemm256x.hip) on GX rows: allowed for this engine / pipeline selected (GLICLASS_MX, glc_debug_set_mx)
    int mx_env = 0;                      // GLICLASS_MX at creation: 0 unset / other, 1 "0", 2 "build" (glc_engine_enable_mx reads it on the ModernBERT backbone)
    float mb_ln_bound = 0.f;             // ModernBERT: max |gamma| sqrt(H) over the norms whose rows become GX operands (the activation exponent glc_engine_enable_mx picks)
    bool mx_ready = false;               // ... and the GX copies of the projection weights exist: built from the split-f16 copies by the first forward that takes the pipeline
    size_t mx_bytes = 0;                 // their size (glc_debug_mx_weight_bytes)
    bool last_mx = false;                // the last forward ran the MX pipeline
    bool last_mx_attn = false;           // ... and its attention ran on MX tiles (attention_mx.hip)
    // MX pipeline for forwards below the 256 tile's fill rule (glc_engine_set_mx_small_forwards / GLICLASS_MX_SMALL; DeBERTa backbone): 0 off,
    // 1 auto (the 128 tile's own fill rule), 2 whenever the shapes allow (tests); their small-M launches run gemm128x.hip
    int mx_small = 0;
    int last_mx128 = 0;                  // GEMM launches of the last forward on the 128 tile
    bool last_rope_epi = false;          // ... and (decoder) its QKV projections ran RoPE + MX tiles as their epilogue (gemm256x EPI_QKVR)
    bool dec_rope_epi = true;            // decoder MX pipeline: RoPE + MX tiles as the QKV projection's epilogue (gemm256x EPI_QKVR); GLC_DEC_ROPE_EPI=0: the separate pass
    bool mx_attn = true;                 // MX pipeline: attention on MX tiles (attention_mx.hip); false: split-f16 units (GLC_MX_ATTN=0, glc_debug_set_mx_attention)
    int debug_stop = -1;                 // developer: leave run_forward after stage (10 * layer + k), k = 0 QKV, 1 attention, 2 attn-out, 3 FFN1, 4 FFN2 (+ LayerNorm): workspace inspection
    int prec_mask = 0;              // precision-budget switches (PM_* of glc_kernels.h; glc_debug_set_precision_mask): operands rounded to f16 in the group-split pipeline
    int gs_mode = 1;                // fp32 mode, group-split activations + 256-tile LDS-DMA GEMMs: 0 off, 1 auto (large shapes), 2 whenever the shapes allow (tests)
    bool last_gs = false;           // the last forward ran the group-split pipeline
    bool ln_fused = true;           // group-split pipeline: LayerNorm folded into the GEMMs around it (GLC_LNF=0: separate LayerNorm kernels)
    bool last_lnf = false;          // the last forward ran with LayerNorm / RMSNorm folded into its GEMMs
    float2 *statsA = nullptr, *statsB = nullptr, *ln_part = nullptr;     // (mean, rstd) per row of X / H1 when they hold raw sums; the producers' partials
    int max_buckets = 4;            // host-buffer forward: split a ragged batch into <= this many length groups (1 = off)
    int last_groups = 1;            // groups the last host-buffer forward ran as
    int range_retries = 0;          // host-buffer forwards repeated with the norms unfused because the folded one came out non-finite
    // fp8 range guard of the MX pipeline (glc_common.h gx_range_note): device counter of activation elements beyond the e4m3 range, its value after the
    // last checked forward, a pinned host slot for the device-resident path; forwards repeated on the split-f16 kernels because they counted
    // any; consecutive such forwards (the model has outlier channels: after kFp8Sticky of them the engine leaves the MX pipeline for good)
    unsigned* d_gxsat = nullptr; unsigned gxsat_seen[2] = {0, 0}; unsigned* h_gxsat = nullptr;      // two words: [0] activation rows (GX images, exponent act_sc), [1] Q / K / V MX tiles (exponent 0)
    int fp8_retries = 0, fp8_streak = 0; bool fp8_sticky_off = false, fp8_device_pending = false;
    int device_invalid = 0;                    // a device-resident forward since the last glc_engine_sync left the fp8 range (1: rows only, 2: tiles): its logits are not valid
    // Activation exponent of the MX pipeline's GX rows (hi8 = e4m3(x 2^act_sc), glc_common.h): 0 until a forward leaves the e4m3 range (|x| > 448);
    // the guard's FIRST answer is then kActScLow = -5 for this engine (rows hold |x| up to 14336, elements below 0.5 keep fewer hi8 bits — their
    // cross terms are 2^-16 of a unit product either way) and the forward is repeated on the MX pipeline; only what still leaves the range
    // (or an MX tile of the attention: Q, K, V, P keep exponent 0) goes to the split-f16 kernels.
    int act_sc = 0;
    float* splitk_ws = nullptr; size_t splitk_ws_bytes = 0;     // fp32 partial tiles of the split-K GEMM path (small M)
    hipStream_t stream = nullptr;
    std::mutex mu;
    std::vector<void*> allocs;      // everything freed at destroy
    // weights
    void* emb = nullptr; float *eln_g = nullptr, *eln_b = nullptr;
    std::vector<LayerW> layers;
    std::vector<DecLayerW> dlayers; float* final_norm = nullptr;      // decoder backbone; ModernBERT: Wgu = Wi, Wd = mlp.Wo, ln1 / ln2 = attn_norm / mlp_norm
    float* zero_bias = nullptr;                                       // ModernBERT: [H] zeros, the beta of its bias-free LayerNorms
    // BERT backbone (layers, eln_g / eln_b as DeBERTa's; the decoder's workspace): the position table [max_positions, H] and row 0 of the
    // token-type table as T, and the position ids [capM] of the forward (rows.hip pos_ids_kernel)
    void *pos_emb = nullptr, *type_emb = nullptr; int* pos_ids = nullptr;
    // T5 backbone (dlayers, final_norm; the decoder's workspace): the bias table rel_bias [rel_buckets, heads] as it came, the per-Sp device
    // tables rpb [t5_heads][2 Sp] = rel_bias[bucket(delta), h] log2(e) at entry delta + Sp - 1 (build_rpb_table), and the head count the
    // kernels run: cfg.heads rounded up to even (the fused QKV projection is a multiple of 128 wide), the extra head all zeros
    std::vector<float> rel_bias; std::map<int, float*> rpbs; int t5_heads = 0;
    std::map<std::pair<int, float>, float*> ropes;                    // (Sp, theta) -> [Sp][d/2][cos,sin]
    void *QKV = nullptr, *GU = nullptr, *X2 = nullptr;                // decoder workspace: fused QKV rows, [gate|up] rows, second residual buffer
    bool fused_swiglu = false;                                        // Wgu rows interleaved 16 gate / 16 up: SwiGLU runs in the GEMM epilogue
    float* headw[8] = {nullptr};
    float* scw[8] = {nullptr};           // the scorer's own tensors (weighted-dot: 8, mlp: 6, simple: none), fp32
    float* scorer_ws = nullptr;          // its row buffers
    float* clsw[GLC_TENSORS_CLS_HEAD] = {nullptr};      // sequence-classification head (head_kind 1): dense.w (pre-split) / .b, norm.w / .b, classifier.w / .b; null = absent
    int P = 0;
    // workspace
    int capM = 0, capB = 0, capIds = 0, capC = 0, capHeadRows = 0, capSel = 0, capGU = 0;
    void *Xs = nullptr, *Qs = nullptr, *CTXs = nullptr, *T1s = nullptr, *H1s = nullptr, *FFs = nullptr;   // compact rows of the pruned last layer
    void* GUs = nullptr;            // ... decoder / ModernBERT: their [first | second] rows of the gated FFN, [Rpad, 2I]
    int *sel_b = nullptr, *sel_q = nullptr;
    unsigned char* tile_flag = nullptr; size_t capFlag = 0;
    void *X = nullptr, *Qh = nullptr, *Kh = nullptr, *Vt = nullptr, *CTX = nullptr, *T1 = nullptr, *H1 = nullptr, *FF = nullptr;
    float* kbias = nullptr; int *klen = nullptr, *kfirst = nullptr, *cls_pos = nullptr, *cls_cnt = nullptr;
    int64_t *d_ids = nullptr, *d_mask = nullptr;
    float *Gt = nullptr, *G1t = nullptr, *G2t = nullptr, *d_logits = nullptr;   // head rows: [text | class] groups, 128-aligned
    std::map<int, int32_t*> dtabs;
    std::map<int, int2*> mtabs;                // Sp -> the MX band kernel's ready-made row offsets (round 6; fp32 mode only): glc_kernels.h AttnArgs::mtab
    std::map<int, int2*> otabs;                // Sp -> byte offsets of the PQ / PK rows per relative distance (band kernel, 16-bit)
    std::map<int, std::pair<int, int>> dsat;   // Sp -> (rsat_pos, rsat_neg)
    // last forward
    int lastB = 0, lastS = 0, lastSp = 0;
    // captured-graph replay of forwards (opt-in: glc_engine_set_graph_replay / GLICLASS_GRAPH_REPLAY=1; engine.hip graph_forward)
    bool graph_on = false;
    bool capturing = false;              // the engine stream is in capture: dmalloc / dfree refuse
    int last_graph = 0;                  // the last forward: 0 eager, 1 captured and launched, 2 replayed
    unsigned long long ws_gen = 0;       // workspace generation: every freed engine buffer bumps it (a cached graph holds the old addresses)
    unsigned long long graph_tick = 0;
    std::vector<GraphEntry> graphs;
    // debug
    bool keep_hidden = false; void* hidden_dump = nullptr; size_t hidden_cap = 0;
    // timing / profile
    hipEvent_t t0 = nullptr, t1 = nullptr;
    bool profile = false;
    struct Ev { hipEvent_t a, b; int cls; };
    std::vector<Ev> evs; size_t ev_used = 0;
    float prof_ms[PC_N] = {0}; int prof_n[PC_N] = {0};
};
