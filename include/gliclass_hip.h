/*
 * gliclass_hip.h — C-ABI of the MI355X (gfx950) GLiClass forward engine ("the HIP shim").
 *
 * This is the boundary the pure-C host code (gliclass/c_amd/host/model.c — the drop-in for
 * /root/reference/src/model.c) binds to.  Plain pointers and sizes only; no C++/torch types.
 * Each entry point names the reference interface it stands in for:
 *
 *   glc_engine_create      <- g_ort->CreateSession(env, model_path, opts, &session)
 *                             /root/reference/src/model.c:269 (graph load + optimise, once)
 *   glc_engine_forward     <- g_ort->Run(session, ..., input_ids, attention_mask -> logits)
 *                             /root/reference/src/model.c:173-182  (the whole hot path)
 *   glc_engine_destroy     <- g_ort->ReleaseSession          /root/reference/main.c:186
 *   glc_delta_table        <- make_log_bucket_position in the exported graph
 *   glc_last_error         <- g_ort->GetErrorMessage(status) /root/reference/src/model.c:194
 *
 * Error convention (mirrors /root/reference/src/model.c): pointer-returning calls return NULL,
 * int-returning calls return non-zero; the message is available from glc_last_error().
 */
#ifndef GLICLASS_HIP_H
#define GLICLASS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* arithmetic type of the GEMM/attention operands (accumulation, LayerNorm statistics, softmax and
 * the scorer head are always fp32) */
enum { GLC_F32 = 0, GLC_BF16 = 1, GLC_F16 = 2 };
enum { GLC_POOL_FIRST = 0, GLC_POOL_AVG = 1, GLC_POOL_LAST = 2 /* last attended token (decoder backbones) */ };
/* scorer of the GLiClass head (upstream `scorer_type`; SURVEY.md §8a row a12 — restated, parity unpinned): 'simple' = dot product of the
 * projected text and class features; 'weighted-dot' = out_mlp([t1, c1, t2 * c2]) on (t1|t2) = proj_text(text), (c1|c2) = proj_label(class),
 * out_mlp = Linear(3H,4H) -> ReLU -> Linear(4H,1); 'mlp' = Linear(2H,256) -> ReLU -> Linear(256,128) -> ReLU -> Linear(128,1) on [text, class] */
enum { GLC_SCORER_DOT = 0, GLC_SCORER_WEIGHTED_DOT = 1, GLC_SCORER_MLP = 2 };
#define GLC_SCORER_MLP_HIDDEN 256
/* backbone family: DeBERTa-v2/v3 disentangled encoder, or a decoder-style stack with Qwen2 / Llama / Qwen3 arithmetic (RMSNorm, RoPE,
 * grouped-query attention, SwiGLU; SURVEY.md §8a row a16, BASELINE.json configs[4]; glc_model_config qk_norm / attn_bias tell the three apart) */
enum { GLC_BACKBONE_DEBERTA = 0, GLC_BACKBONE_DECODER = 1,
       GLC_BACKBONE_MODERNBERT = 2 /* ModernBERT encoder: LayerNorm without bias, RoPE, bidirectional attention with a sliding window on the
                                      local layers, GeGLU (transformers models/modernbert/modeling_modernbert.py) */,
       GLC_BACKBONE_BERT = 3 /* BERT / RoBERTa / XLM-R encoder: learned absolute position embeddings (+ token-type row 0), post-LayerNorm blocks
                                with biases, plain bidirectional attention, erf-GELU FFN (transformers models/bert/modeling_bert.py,
                                models/roberta/modeling_roberta.py) */,
       GLC_BACKBONE_T5 = 4 /* T5 v1.1 / mT5 / flan-T5 encoder (transformers models/t5/modeling_t5.py, the encoder T5Stack): pre-norm blocks on
                              bias-free RMSNorms and projections, attention without the 1/sqrt(d) scale and with a learned per-head bias
                              indexed by the bucket of key - query (layer 0's table, shared by every layer), gated tanh-GELU FFN; heads *
                              head_dim need not be the hidden size */ };

/* Same int/float slots, same order, as the .glcw blob header (gliclass/c_amd/weights.py). */
typedef struct glc_model_config {
    int32_t vocab, hidden, layers, heads, head_dim, inter, pos_buckets, max_rel_pos;
    int32_t pad_id, cls_id, sep_id, class_token_index, text_token_index;
    int32_t pooling, scorer, embed_class_token, normalize_features;
    int32_t backbone, kv_heads, causal;    /* decoder backbone: key/value heads (0 = heads), causal mask on/off */
    float ln_eps, logit_scale;             /* ln_eps is rms_norm_eps for the decoder backbone */
    float rope_theta;                      /* ModernBERT: the global layers' base */
    /* ModernBERT: local layers attend to keys with |q - k| <= local_window (0 = every layer global); layer l is global when
     * l % global_every == 0; rope_theta_local is the local layers' RoPE base */
    int32_t local_window, global_every;
    float rope_theta_local;
    /* decoder backbone: qk_norm = 1 applies an RMSNorm over head_dim (gains q_norm / k_norm, epsilon ln_eps) to every query and key head
     * before RoPE (Qwen3); attn_bias = 0 drops the q / k / v projection biases (Llama, Qwen3).  Qwen2 is (0, 1), and so is every other backbone. */
    int32_t qk_norm, attn_bias;
    /* BERT backbone: rows of the position table (max_position_embeddings) and of the token-type table; pos_offset = 0 numbers the positions
     * 0 .. S-1 (BERT), pos_offset = pad_id + 1 numbers the non-pad tokens from pos_offset on and gives pad tokens row pad_id (RoBERTa / XLM-R,
     * create_position_ids_from_input_ids).  A forward takes at most max_positions - pos_offset tokens per row.  0 on every other backbone. */
    int32_t max_positions, type_vocab, pos_offset;
    /* T5 backbone: relative_attention_num_buckets and relative_attention_max_distance of the bias table (bidirectional buckets).  0 on every
     * other backbone. */
    int32_t rel_buckets, rel_max_distance;
    /* Head kind: GLC_HEAD_GLICLASS (0, every field below 0) or GLC_HEAD_SEQCLS, the head of an HF *ForSequenceClassification checkpoint on the
     * DeBERTa, BERT and ModernBERT backbones (refused on the decoder and T5 backbones): pooled row ('first' or 'avg' pooling) -> [dense H x H ->]
     * activation -> [LayerNorm, epsilon ln_eps ->] classifier, fp32 logits [B, cls_labels].  cls_labels = K in 1 .. 1024; cls_act: GLC_CLS_ACT_*;
     * cls_norm / cls_dense: 0 / 1.  The class-token and scorer fields are not read by this head. */
    int32_t head_kind, cls_labels, cls_act, cls_norm, cls_dense;
} glc_model_config;
enum { GLC_HEAD_GLICLASS = 0, GLC_HEAD_SEQCLS = 1 };
enum { GLC_CLS_ACT_NONE = 0, GLC_CLS_ACT_TANH = 1, GLC_CLS_ACT_GELU = 2 /* erf form */ };
#define GLC_CLS_MAX_LABELS 1024

/* Tensor order expected in `tensors[]` (all fp32, row-major, nn.Linear weights are [out,in]):
 *   0 embeddings.word_embeddings.weight [vocab,H]      1,2 embeddings.LayerNorm.{weight,bias}
 *   3 encoder.rel_embeddings.weight [2*span,H]         4,5 encoder.LayerNorm.{weight,bias}
 *   6+16*l .. : layer l: q.w q.b k.w k.b v.w v.b  attn.out.w attn.out.b attn.LN.w attn.LN.b
 *                        inter.w inter.b  out.w out.b out.LN.w out.LN.b
 *   then text_projector.linear_1.{w,b} linear_2.{w,b}, classes_projector.linear_1.{w,b} linear_2.{w,b}
 *   then the scorer's tensors (none for 'simple'):
 *     weighted-dot: scorer.proj_text.{weight [2H,H], bias [2H]}  scorer.proj_label.{weight [2H,H], bias}
 *                   scorer.out_mlp.0.{weight [4H,3H], bias [4H]}  scorer.out_mlp.3.{weight [1,4H], bias [1]}
 *     mlp:          scorer.mlp.0.{weight [256,2H], bias}  scorer.mlp.2.{weight [128,256], bias}  scorer.mlp.4.{weight [1,128], bias [1]} */
#define GLC_TENSORS_FIXED 6
#define GLC_TENSORS_PER_LAYER 16
#define GLC_TENSORS_HEAD 8
static inline int glc_num_tensors(int layers) { return GLC_TENSORS_FIXED + GLC_TENSORS_PER_LAYER * layers + GLC_TENSORS_HEAD; }
static inline int glc_num_scorer_tensors(int scorer) { return scorer == GLC_SCORER_WEIGHTED_DOT ? 8 : scorer == GLC_SCORER_MLP ? 6 : 0; }
/* Decoder backbone (names of HF Qwen2Model / LlamaModel / Qwen3Model.state_dict()):
 *   0 embed_tokens.weight [vocab,H]
 *   1+n*l .. : layer l: input_layernorm.weight  q_proj.weight [nq*d,H] (q_proj.bias)  k_proj.weight [nkv*d,H] (k_proj.bias)
 *                       v_proj.weight (v_proj.bias)  [self_attn.q_norm.weight [d]  self_attn.k_norm.weight [d]]
 *                       o_proj.weight [H,nq*d]  post_attention_layernorm.weight
 *                       mlp.gate_proj.weight [I,H]  mlp.up_proj.weight [I,H]  mlp.down_proj.weight [H,I]
 *     (...) only with attn_bias, [...] only with qk_norm; n = glc_dec_tensors_per_layer: 12 for Qwen2, 9 for Llama, 11 for Qwen3
 *   then norm.weight [H], then the same 8 head tensors */
#define GLC_DEC_TENSORS_PER_LAYER 12
static inline int glc_dec_tensors_per_layer(const glc_model_config* c) { return GLC_DEC_TENSORS_PER_LAYER - (c->attn_bias ? 0 : 3) + (c->qk_norm ? 2 : 0); }
/* ModernBERT backbone (names of HF ModernBertModel.state_dict(); no biases anywhere):
 *   0 embeddings.tok_embeddings.weight [vocab,H]       1 embeddings.norm.weight [H]
 *   then per layer l: layers.l.attn_norm.weight [H] (only for l > 0; layer 0's is the identity)
 *                     attn.Wqkv.weight [3H,H] (rows: Q | K | V, head-major)  attn.Wo.weight [H,H]
 *                     mlp_norm.weight [H]  mlp.Wi.weight [2I,H] (rows: input | gate)  mlp.Wo.weight [H,I]
 *   then final_norm.weight [H], then the same 8 head tensors */
#define GLC_MB_TENSORS_PER_LAYER 6
/* BERT backbone (names of HF BertModel / RobertaModel / XLMRobertaModel.state_dict() except the fused attention projection; the pooler is ignored):
 *   0 embeddings.word_embeddings.weight [vocab,H]      1 embeddings.position_embeddings.weight [max_positions,H]
 *   2 embeddings.token_type_embeddings.weight [type_vocab,H]      3,4 embeddings.LayerNorm.{weight,bias}
 *   5+12*l .. : layer l: attention.self.Wqkv.weight [3H,H] (rows: query | key | value, concatenated by the importers)  attention.self.Wqkv.bias [3H]
 *                        attention.output.dense.{weight,bias}  attention.output.LayerNorm.{weight,bias}
 *                        intermediate.dense.{weight [I,H],bias}  output.dense.{weight [H,I],bias}  output.LayerNorm.{weight,bias}
 *   then the same 8 head tensors */
#define GLC_BERT_TENSORS_FIXED 5
#define GLC_BERT_TENSORS_PER_LAYER 12
/* T5 backbone (names of HF T5EncoderModel.state_dict() except the fused attention projection; no biases anywhere; inner = heads * head_dim):
 *   0 shared.weight [vocab,H]      1 encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight [rel_buckets,heads]
 *   2+6*l .. : block l: layer.0.layer_norm.weight [H]  layer.0.SelfAttention.Wqkv.weight [3*inner,H] (rows: q | k | v, concatenated by the importers)
 *                       layer.0.SelfAttention.o.weight [H,inner]  layer.1.layer_norm.weight [H]
 *                       layer.1.DenseReluDense.Wgu.weight [2I,H] (rows: wi_0 | wi_1, concatenated by the importers)  layer.1.DenseReluDense.wo.weight [H,I]
 *   then encoder.final_layer_norm.weight [H], then the same 8 head tensors */
#define GLC_T5_TENSORS_FIXED 2
#define GLC_T5_TENSORS_PER_LAYER 6
/* Sequence-classification head (head_kind = GLC_HEAD_SEQCLS): behind the backbone tensors, IN PLACE of the 8 projector tensors and the scorer's,
 * always GLC_TENSORS_CLS_HEAD slots (all fp32; the arithmetic with its transformers sources is in csrc/cls_head.hip):
 *   0 dense.weight [H,H]   1 dense.bias [H]                 both NULL when cls_dense = 0; dense.bias alone may be NULL (ModernBERT classifier_bias = false)
 *   2 norm.weight [H]      3 norm.bias [H]                  both NULL when cls_norm = 0; norm.bias alone may be NULL (ModernBERT norm_bias = false)
 *   4 classifier.weight [K,H]   5 classifier.bias [K]       the bias may be NULL
 * A NULL slot is a tensor the checkpoint does not have; every other tensor of the list must be present.  Blob names: the same with the prefix
 * "cls." (gliclass/c_amd/weights.py); a version-7 blob records only the tensors that exist.
 * This is the first head of the repository whose logits are pinned end to end on transformers' own numbers (tests/golden/seqcls). */
#define GLC_TENSORS_CLS_HEAD 6
static inline int glc_num_head_tensors(const glc_model_config* c) {
    return c->head_kind == GLC_HEAD_SEQCLS ? GLC_TENSORS_CLS_HEAD : GLC_TENSORS_HEAD + glc_num_scorer_tensors(c->scorer);
}
/* tensors of a configuration with the GLiClass head (the backbone's, the 8 projector tensors, the scorer's) */
static inline int glc_num_tensors_gliclass(const glc_model_config* c) {
    if (c->backbone == GLC_BACKBONE_T5)
        return GLC_T5_TENSORS_FIXED + GLC_T5_TENSORS_PER_LAYER * c->layers + 1 + GLC_TENSORS_HEAD + glc_num_scorer_tensors(c->scorer);
    if (c->backbone == GLC_BACKBONE_BERT)
        return GLC_BERT_TENSORS_FIXED + GLC_BERT_TENSORS_PER_LAYER * c->layers + GLC_TENSORS_HEAD + glc_num_scorer_tensors(c->scorer);
    if (c->backbone == GLC_BACKBONE_MODERNBERT)
        return 3 + GLC_MB_TENSORS_PER_LAYER * c->layers - (c->layers > 0 ? 1 : 0) + GLC_TENSORS_HEAD + glc_num_scorer_tensors(c->scorer);
    return (c->backbone == GLC_BACKBONE_DECODER ? 2 + glc_dec_tensors_per_layer(c) * c->layers + GLC_TENSORS_HEAD : glc_num_tensors(c->layers)) +
           glc_num_scorer_tensors(c->scorer);
}
/* ... and of any configuration: the sequence-classification head's slots stand in place of the projector and scorer tensors */
static inline int glc_num_tensors_cfg(const glc_model_config* c) {
    return c->head_kind == GLC_HEAD_SEQCLS ? glc_num_tensors_gliclass(c) - GLC_TENSORS_HEAD - glc_num_scorer_tensors(c->scorer) + GLC_TENSORS_CLS_HEAD
                                           : glc_num_tensors_gliclass(c);
}
/* index of layer l's first tensor (attn_norm for l > 0, Wqkv for l = 0) in the ModernBERT order */
static inline int glc_mb_layer_base(int l) { return l == 0 ? 2 : 2 + GLC_MB_TENSORS_PER_LAYER * l - 1; }

typedef struct glc_engine glc_engine;

int glc_device_count(void);
const char* glc_last_error(void);

/* Uploads + converts weights, precomputes LayerNorm(rel_embeddings) and the per-layer position
 * projections (batch independent).  `device` = HIP ordinal.  Host tensors may be freed afterwards. */
glc_engine* glc_engine_create(const glc_model_config* cfg, const float* const* tensors, int n_tensors,
                              int device, int dtype);
void glc_engine_destroy(glc_engine* e);

/* Host-buffer forward: ids/mask int64 [B,S] row-major (what create_tensor() wraps,
 * /root/reference/src/model.c:39-71).  Writes logits[b*c_alloc + j], j < *c_out, where
 * *c_out = max over rows of the number of class tokens (the ONNX graph's dynamic C).
 * Blocking; thread-safe per engine (internally serialised, cf. /root/reference/main.c:143-146). */
int glc_engine_forward(glc_engine* e, const int64_t* ids, const int64_t* mask, int B, int S,
                       float* logits, int c_alloc, int* c_out);
/* Sequence-classification engines (head_kind = GLC_HEAD_SEQCLS): the same two forwards write logits [B, K], K = cls_labels.  glc_engine_forward
 * needs c_alloc >= K, writes logits[b*c_alloc + k], k < K (with c_alloc > K the columns k >= K are unspecified), and sets *c_out = K; glc_engine_forward_device needs C == K.  Both fail with a message
 * otherwise.  The inputs need no <<LABEL>> tokens: class tokens are still scanned for, and what the scan finds is not used. */

/* Device-resident forward (bench / pipelined callers): d_ids, d_mask int64 [B,S] and d_logits
 * f32 [B,C] are device pointers on this engine's device; C = number of class-token slots to score.
 * Enqueues on the engine stream and returns; call glc_engine_sync() to wait.
 *
 * CONTRACT (fp8 range guard of the MX pipeline, the default arithmetic of large fp32-mode forwards): the operand images of that pipeline
 * hold e4m3 parts; an activation beyond their range (|x| > 448) has no image, and from 464 on its parts are NaN.  A host-buffer forward
 * (glc_engine_forward) notices and repeats itself behind the caller's back; a device-resident forward cannot.  Its d_logits are valid
 * only once glc_engine_sync() has returned 0 — or glc_engine_device_forward_valid() has returned 1 for callers that wait by other means.
 * glc_engine_sync() returning -1 with "... run the forward again" means: the logits of the forward(s) since the last sync are NOT valid,
 * the engine has already changed its arithmetic (first answer: activation rows at exponent -5, |x| up to 14336, still on the MX pipeline;
 * second answer, or outliers in Q / K / V: the split-f16 kernels for good, as GLICLASS_MX=0), and the same forward has to be enqueued again.
 * At most two such repeats per engine lifetime.  Consumers queued on the stream BEHIND the forward (an RCCL all-gather, a D2H copy) read
 * whatever the forward wrote: check before trusting them.  Engines created with GLICLASS_MX=0, 16-bit engines and small forwards never
 * take the MX pipeline and never report this.  A ModernBERT engine takes the MX pipeline only after glc_engine_enable_mx (below) and reports the
 * fp8 range through glc_engine_sync from then on, like the other backbones; without that call it never does. */
int glc_engine_forward_device(glc_engine* e, const void* d_ids, const void* d_mask, int B, int S, int C,
                              void* d_logits);
int glc_engine_sync(glc_engine* e);
int glc_engine_device_forward_valid(glc_engine* e);      /* 1 valid / 0 repeat the forward / -1 error; the stream must be idle (see above) */

/* Zero-shot NLI scores on the device (semantics of transformers/pipelines/zero_shot_classification.py postprocess): d_logits f32 [T*Lb, K] are the
 * logits of the T*Lb (text, hypothesis) pairs, pair (t, l) in row t*Lb + l — what a forward of this engine wrote for that pair batch —, d_probs
 * f32 [T, Lb] the result; both device pointers on this engine's device.  multi_label = 1: per pair, softmax over the two logits (contra_id,
 * entail_id) and the entailment share; multi_label = 0: per text, softmax of the entail_id logits over its Lb labels (contra_id is not read).
 * Max-subtracted exp2 in fp32.  Enqueues on the engine's stream and returns: glc_engine_sync() (or a glc_memcpy_d2h, which is ordered behind
 * it on that stream) before the host reads d_probs.  Returns 0; -1 with a message in glc_last_error() for a null engine or pointer, a
 * GLiClass-head engine, K < 2, T < 1, Lb < 1, or entail_id / contra_id outside 0 .. K-1 (multi_label = 1: also entail_id == contra_id). */
int glc_engine_nli_scores(glc_engine* e, const float* d_logits, int T, int Lb, int entail_id, int contra_id, int multi_label, float* d_probs);

/* Opt-in MX pipeline of the ModernBERT backbone (the DeBERTa and decoder backbones take theirs by default).  Builds the GX copies of the four
 * projection weights of every layer and selects the pipeline: large fp32-mode forwards (the group-split ones) then run their projections on
 * the MX cross-term GEMM (GeGLU in its epilogue) and their attention on MX tiles (global layers: the K / V^T ring kernel; local layers: the
 * windowed per-wave kernel).  Returns 0, or -1 with a message in glc_last_error() naming the condition that failed: fp32 dtype; split-f16
 * weights and attention (no GLICLASS_F32_GEMM / GLICLASS_F32_ATTN = native); no GLICLASS_MX=0; hidden % 256 == 0; (2 inter) % 256 == 0 and
 * inter % 32 == 0 (modernbert-large, 2 x 2624 = 5248, is not eligible); head_dim 64; not under glc_debug_keep_hidden.  The activation
 * exponent is chosen here from the LayerNorm gains (max |gamma| sqrt(hidden) > 448: exponent -5 from the start).  Afterwards GLICLASS_MX=build,
 * glc_debug_set_mx, glc_debug_set_mx_attention, the glc_debug_last_forward_mx* queries and the fp8 range guard behave as on the decoder
 * backbone.  On the other backbones: 0 if the MX pipeline is available to the engine, else -1; nothing changes (the BERT and T5 backbones
 * have no MX pipeline: always -1, the message says so).
 * Environment: GLICLASS_MX_MODERNBERT=1, read once in glc_engine_create, makes this call for a ModernBERT engine (a failure leaves the
 * engine as it is and is not an error). */
int glc_engine_enable_mx(glc_engine* e);

/* Captured-graph replay of forwards (opt-in, default 0): for callers that send the same (B, S, C) shapes again and again.  It takes the
 * host's submission cost of a forward (a hundred and more launches) down to one call.  MEASURED (profiles/graph_replay/summary.txt): with
 * forwards enqueued back to back the device's own time per launch bounds a small forward, not the submission, and replay is 0.5-1 % SLOWER
 * at B = 8.  The host's time per call and the latency of a single awaited forward have not been measured.  Leave it off unless you have
 * measured your own caller.
 * Per key — backbone, B, S, padded S, C, every pipeline switch, the workspace generation and the three device pointers (the caller's on
 * glc_engine_forward_device; the engine's own staging buffers on glc_engine_forward, each group of a length-bucketed forward its own key) —
 * the first forward runs as always, the second is captured on the engine's stream as a HIP graph (one linear chain) and launched, later ones
 * are one hipGraphLaunch.  Results are bit-identical: the graph holds the same launches on the same buffers and reads the ids, the mask,
 * the class-token positions and the range guard's counter from device memory at every replay.  H2D / D2H copies of the host-buffer entry,
 * the fp8 range guard's read and its repeats stay outside the graph and work as before.  Forwards under glc_profile_enable,
 * glc_debug_keep_hidden or glc_debug_set_stop, and a key whose capture failed, run eagerly.  Every glc_engine_set_* / glc_debug_set_* call,
 * glc_engine_enable_mx, glc_profile_enable, glc_debug_keep_hidden, a workspace buffer that moves (a larger shape) and every answer of the range
 * guards drop all cached graphs; at most 16 are kept per engine (least recently used goes first).  A device-resident caller must keep
 * d_ids / d_mask / d_logits alive while the engine may replay them: free them only after switching replay off, destroying the engine, or any
 * of the calls above.  Returns 0; -1 (glc_last_error) for a null engine.  Turning it off drops every cached graph.
 * Environment: GLICLASS_GRAPH_REPLAY=1, read once in glc_engine_create, makes this call (a failure leaves the engine eager, not an error). */
int glc_engine_set_graph_replay(glc_engine* e, int on);
int glc_debug_last_forward_graph(const glc_engine* e);     /* the last forward: 0 ran eagerly (warm-up and ineligible forwards included), 1 was captured and launched, 2 replayed a cached graph (length-bucketed: the minimum over its groups); -1: null engine */
int glc_debug_graph_cache_size(const glc_engine* e);       /* graph executables the engine holds (0 .. 16); -1: null engine */

/* MX pipeline for mid-size forwards (opt-in, default 0; DeBERTa backbone, fp32 mode).  Which arithmetic an fp32-mode forward gets is decided by
 * one fill rule, (Mpad / 256) (H / 256) 2 >= CUs: at or above it the group-split / MX pipeline (two matrix-pipe units per product), below it
 * the 128-tile split-K kernels on split-f16 operands (three units).  With mode >= 1 a forward that fails ONLY that rule is still admitted to
 * the group-split + MX pipeline, and its GEMM launches with too few 256-tiles for the device run the 128 x 128 tile of the MX GEMM
 * (csrc/gemm128x.hip: same operands, same arithmetic order, outputs bit-identical to the 256 tile's).  Every other condition of the pipeline
 * stays: pruned last layer, split-f16 weights and attention, hidden % 256 == 0, inter % 256 == 0, folded LayerNorm, layers >= 2, no
 * precision mask, MX weight copies buildable.
 *   mode 0  off: every decision exactly as without this call
 *   mode 1  auto: admitted when the same fill rule holds for the 128 tile, (Mpad / 128) (H / 128) 2 >= CUs (256 CUs, H = 768: from ~2.8 k rows)
 *   mode 2  whenever the shapes allow (tests)
 * PRECISION: a forward taken by the switch moves from the split-f16 arithmetic (~1e-5 per-label probability error against the oracle) to the MX
 * arithmetic's ~4e-5 — the error large forwards have by default; that is why it is opt-in.  The fp8 range guard, its retries and
 * glc_engine_sync's report apply unchanged.  Speed: not measured yet; nothing is promised.
 * Changing the mode drops every cached graph.  Returns 0; -1 (glc_last_error) for a null engine, a mode outside 0 .. 2, or mode >= 1 on the
 * decoder / ModernBERT / BERT / T5 backbones (the message names the backbone; mode 0 returns 0 there).
 * Environment: GLICLASS_MX_SMALL=1|2, read once in glc_engine_create, makes this call (a failure leaves the engine as it is, not an error). */
int glc_engine_set_mx_small_forwards(glc_engine* e, int mode);
int glc_debug_last_forward_mx128(const glc_engine* e);     /* GEMM launches of the last forward that ran on the 128 tile (0: none); -1: null engine */

/* Exact last-layer pruning (default on; env GLICLASS_PRUNE_LAST=0 disables), on every backbone: the final layer computes attention
 * output, output projection and FFN (DeBERTa: Q as well) only for the rows the head reads — the pooled row of each sequence ([CLS] /
 * position 0, or the last attended token with 'last' pooling) and its class tokens; K and V are still made for every position.  Logits
 * are unchanged.  Never with average pooling (it reads every row) and never under glc_debug_keep_hidden (it dumps every row).
 * Not on the BERT backbone: its last layer runs on every row and glc_debug_last_forward_pruned answers 0 (post-LayerNorm pruning on the
 * compact path is a follow-up); the switch is accepted and has no effect there. */
int glc_engine_set_prune_last_layer(glc_engine* e, int on);
int glc_debug_last_forward_pruned(const glc_engine* e);        /* 1: the last forward ran that compact last layer, 0: it did not, -1: null engine */

/* Length bucketing of glc_engine_forward (host buffers): the reference pads every row of a batch to the longest one
 * (/root/reference/src/tokenizer.c:44-54); rows are independent, so a ragged batch is run as up to `max_groups` groups of
 * similar length, each padded to its own longest row (results per row are unchanged; only padding work is saved).
 * Default 4 (env GLICLASS_LENGTH_BUCKETS), 1 = off.  The device-resident forward is never bucketed. */
int glc_engine_set_length_buckets(glc_engine* e, int max_groups);
/* The planner on its own (host only, no GPU): rows sorted longest first into `order` [B]; group g = order[cuts[g] .. cuts[g+1]);
 * cuts has *n_groups + 1 entries (caller provides B + 1).  Cost model (engine.hip): padded token rows rounded up to whole waves of
 * 256-row GEMM tiles over the CUs for the N = hidden projections, plus 1024 rows per group. */
int glc_plan_length_buckets(const int* lengths, int B, int max_groups, int hidden, int* order, int* cuts, int* n_groups);
int glc_debug_last_forward_groups(const glc_engine* e);   /* how many length groups the last glc_engine_forward ran as */

/* Device memory helpers so a host language can stage buffers without linking HIP itself. */
void* glc_device_malloc(glc_engine* e, size_t bytes);
void glc_device_free(glc_engine* e, void* p);
int glc_memcpy_h2d(glc_engine* e, void* dst, const void* src, size_t bytes);
int glc_memcpy_d2h(glc_engine* e, void* dst, const void* src, size_t bytes);

/* HIP-event timing on the engine stream (the stream every kernel is launched on). */
int glc_timer_start(glc_engine* e);
float glc_timer_stop_ms(glc_engine* e); /* records, synchronises, returns elapsed ms (<0 on error) */

/* Per-kernel-class profile: when enabled every launch is bracketed by HIP events.
 * glc_profile_read returns the number of classes and fills name/total_ms/launch counts. */
#define GLC_PROFILE_MAX 16
int glc_profile_enable(glc_engine* e, int on);
int glc_profile_read(glc_engine* e, const char** names, float* total_ms, int* launches, int max_n);

/* Diagnostics for parity tests: copy a hidden state of the LAST forward to host as fp32
 * [B,S,H]; which = 0 embeddings output, l+1 = output of layer l.  Only valid after
 * glc_debug_keep_hidden(e,1) was set before the forward. */
int glc_debug_keep_hidden(glc_engine* e, int on);
int glc_debug_get_hidden(glc_engine* e, int which, float* out, size_t out_elems);
/* Attention kernel choice: 0 auto, 1 straightforward (non-MFMA), 2 per-wave MFMA band kernel, 3 workgroup-shared band kernel. */
int glc_debug_set_attention_impl(glc_engine* e, int impl);

/* fp32 mode: the group-split pipeline (activations kept as [32 hi | 32 lo] f16 groups, every projection on the 256-tile LDS-DMA
 * kernel).  mode 0 off, 1 auto (default: forwards large enough to fill the chip), 2 whenever the shapes allow (tests). */
int glc_debug_set_group_split(glc_engine* e, int mode);
int glc_debug_last_forward_group_split(const glc_engine* e);
/* MX cross-term pipeline (docs/LOG_r01-r05.md §3e): every projection of the full layers as a_hi*w_hi in f16 MFMAs + both cross terms in ONE
 * block-scaled fp8 MFMA, on "GX" rows.  Needs the GX weight copies, i.e. an engine created under GLICLASS_MX=1 (selected) or =build. */
int glc_debug_set_mx(glc_engine* e, int on);
int glc_debug_last_forward_mx(const glc_engine* e);
int glc_debug_last_forward_mx_attention(const glc_engine* e);   /* 1: the last forward's attention ran on MX tiles (two MFMA times per product) */
int glc_debug_last_forward_rope_epilogue(const glc_engine* e);  /* 1: (decoder) its QKV projections ran RoPE + MX tiles as their epilogue (EPI_QKVR): never with qk_norm */
int glc_debug_set_mx_attention(glc_engine* e, int on);                 /* MX pipeline: attention on MX tiles (default) / on split-f16 units */
long long glc_debug_mx_weight_bytes(const glc_engine* e);  /* bytes of the GX weight copies (0 until a forward has taken the MX pipeline: they are built then) */
/* Developer: stop forwards after a stage (engine.hip) and read workspace rows decoded to fp32 (engine_debug.hip). */
int glc_debug_set_stop(glc_engine* e, int stage);
int glc_debug_read_workspace(glc_engine* e, int which, int rows, float* out);
/* BERT backbone: the position ids [B, Sp] (Sp = S rounded up to 64) of the last forward, as the embedding kernel read them; n = B * Sp */
int glc_debug_read_pos_ids(glc_engine* e, int32_t* out, int n);
/* Group-split pipeline: LayerNorm folded into the GEMMs around it (1, default: the producer writes raw rows + row statistics, the consumer
 * runs on weights with gamma folded in and finishes (LN(x) W^T + b) in its epilogue) or as kernels of its own (0). */
int glc_debug_set_ln_fused(glc_engine* e, int on);
int glc_debug_last_forward_ln_folded(const glc_engine* e);      /* 1: the last forward ran with the norm folded into its GEMMs (every mode) */
/* Precision budget of the default mode (developer; scripts/precision_budget.py): a set bit rounds one operand group of the group-split
 * pipeline to f16 by dropping its lo halves — numerically the cheaper kernel that never fetches them.  Bits 0-7: (A, W) of the QKV,
 * attention-output, FFN1, FFN2 projections; 8-13: attention Q, K, V^T, P, PQ rows, PK rows; 14: the residual rows. */
int glc_debug_set_precision_mask(glc_engine* e, int mask);
/* Host-buffer forwards that were repeated with the norms unfused because the folded forward came out non-finite (a raw residual
 * stream beyond the f16 operand range; engine.hip forward_one). */
int glc_debug_range_retries(const glc_engine* e);
/* fp8 range guard of the MX pipeline: host-buffer forwards repeated on the split-f16 kernels because an activation left the e4m3 range of the
 * operand images (|x| > 448); 1 once the engine has left the MX pipeline for good (two such host-buffer forwards in a row; a device-resident forward
 * whose Q / K / V tiles left the range, or a second one after the activation exponent was already lowered — glc_engine_sync's second answer) */
int glc_debug_fp8_range_retries(const glc_engine* e);
int glc_debug_fp8_range_sticky(const glc_engine* e);
/* ... and the exponent the engine's activation rows carry: 0, or -5 once a forward left the range (the guard's first answer: rows that hold
 * |x| up to 14336, the forward repeated on the MX pipeline; only what still leaves the range goes to the split-f16 kernels) */
int glc_debug_activation_exponent(const glc_engine* e);
/* 256-tile GEMM ring: full-line (operand-major) stages on / off, process-wide developer A/B switch; bit-identical results. */
int glc_debug_set_gemm_full_lines(int on);

/* clamp(bucket(q-k)+span, 0, 2span-1) for q-k in [-(S-1), S-1] at out[q-k+S-1] (float32 math as
 * torch).  Pure host function (no GPU needed). */
void glc_delta_table(int S, int bucket_size, int max_position, int32_t* out);
/* T5 backbone: T5Attention._relative_position_bucket (bidirectional) of delta = key - query for delta in [-(S-1), S-1] at out[delta + S - 1]:
 * half the buckets for delta > 0, distances below num_buckets / 4 exact, beyond them float32 log spacing up to max_distance, truncated and
 * clamped (float32 math as torch).  Pure host function (no GPU needed). */
void glc_t5_bucket_table(int S, int num_buckets, int max_distance, int32_t* out);

/* Developer microbenchmark of one GEMM shape (16-bit engines): ms per launch, <0 on error. */
float glc_debug_gemm_bench(glc_engine* e, int M, int N, int K, int epi, int iters, int which);
/* Kernel-level tests (tests/test_gpu_gemm_kernels.py; tests/test_gpu_mx.py: the MX cross-term GEMM against the split-f16 GEMM on the same
 * operands, two calls per case): ONE launcher call of one GEMM kernel on operands the caller chose.
 * The host fp32 operands are encoded with the library's own converters (glc_launch_convert / _presplit / _to_gx / _gs_to_gx), the launcher
 * runs once, and the RAW BYTES of every output, of ln_part, of the encoded operand images and the two words of the fp8 range counter come
 * back; decoding them is the caller's business (tests/gemm_ref.py: a second reading of the formats).  Every output sits between two guard
 * regions and is, like them, prefilled with the byte `fill`.  A shape the launcher (or, before it, one of the converters) refuses returns -2
 * with its message in glc_last_error() and no GEMM launched; -1 = bad arguments or a HIP error. */
enum { GLC_GEMM_RUN_128 = 0,     /* gemm.hip, the engine's dtype (fp32 engines: the split-f16 path; w_presplit = W split at load) */
       GLC_GEMM_RUN_256S = 1,    /* gemm256s.hip, 16-bit engines */
       GLC_GEMM_RUN_GS = 2,      /* gemm256s.hip on group-split rows */
       GLC_GEMM_RUN_MX = 3,      /* gemm256x.hip on GX rows */
       GLC_GEMM_RUN_AUTO = 4,    /* glc_launch_gemm_auto, the engine's dtype */
       GLC_GEMM_RUN_MX128 = 5 }; /* gemm128x.hip on GX rows: operands encoded as for GLC_GEMM_RUN_MX */
typedef struct glc_gemm_run {
    /* ---- in ---- */
    int32_t kernel, epi;                               /* GLC_GEMM_RUN_*; EPI_* of csrc/glc_kernels.h (0 bias, 1 GELU, 2 residual, 3 QKV, 4 SwiGLU, 5 QKVR, 6 GeGLU) */
    int32_t Mpad, N, K;
    const float *A, *W, *bias, *W2, *bias2, *resid;    /* host fp32: A [Mpad,K], W / W2 [N,K], bias / bias2 [N], resid [Mpad,N]; null = absent */
    const float *a_stats, *ln_c, *r_stats, *r_gamma, *r_beta, *rope_cs;   /* a_stats / r_stats [Mpad] (x, y) pairs; ln_c, r_gamma, r_beta [N]; rope_cs [Sp][64] (cos, sin) */
    const unsigned char* q_tile_flag;                  /* [Mpad / 32] */
    int32_t m_split, Mvalid, Sp, nh, H, nq, nkv;
    float qscale;
    int32_t qkv_skip_q, qkv_split, qkv_mxt, gs_c_plain, gs_resid_plain, perm_cols, prec, mx_ws, act_sc, gx_rows;
    int32_t w_presplit;                                /* GLC_GEMM_RUN_128 on an fp32 engine: W (and W2) through glc_launch_presplit, as the engine loads them */
    int32_t w_from_gs;                                 /* GLC_GEMM_RUN_MX: W through glc_launch_presplit + glc_launch_gs_to_gx (the engine's path) instead of glc_launch_to_gx */
    int32_t glu_interleaved;                           /* GLC_GEMM_RUN_MX, GeGLU: the caller states that W's rows interleave 16 input / 16 gate features (GemmArgs::glu_interleaved); 0: refused */
    int32_t want_ln_part;                              /* pass an ln_part buffer [Mpad][N / 64] (x, y) */
    int32_t fill;                                      /* byte the outputs, ln_part and the guards are prefilled with */
    uint64_t ws_bytes;                                 /* split-K workspace of the 128-tile kernel; 0 = none */
    /* ---- out (host buffers of the caller; a null pointer skips that copy) ---- */
    void* out[3]; uint64_t out_bytes[3];               /* C, or Qh / Kh / Vt: capacity, at least the bytes of that output (engine_debug.hip gemm_run_out_bytes) */
    void* ln_part;                                     /* Mpad * (N / 64) * 8 bytes */
    void *A_img, *W_img, *W2_img, *resid_img;          /* the encoded operands: element bytes (2, or 4 for fp32 / GS / GX) x count */
    uint32_t sat[2];                                   /* the fp8 range counter after the launch */
    int32_t guards_ok;                                 /* 1: every guard region still holds `fill` */
    int32_t cus;                                       /* compute units of the engine's device: what the split-K part count and the small-M rule of the launchers depend on */
} glc_gemm_run;
int glc_debug_gemm_run(glc_engine* e, glc_gemm_run* r);
/* glc_launch_ln_stats on host partials part [M][nparts] (sum, M2) -> stats [M] (mean, rstd) pairs; rms: (0, 1 / sqrt(E[x^2] + eps)) */
int glc_debug_ln_stats_run(glc_engine* e, const float* part, int nparts, int M, float eps, int rms, float* stats);
/* Developer microbenchmark of the band attention kernel on the workspace of the last forward (see engine_debug.hip). */
float glc_debug_attn_bench(glc_engine* e, int iters, int variant, int stamps, double* checksum);
int glc_debug_is_developer_build(void);                  /* 1: built with make DEV=1 (developer kernels, stamps, GLC_* switches); 0: the product library */

const glc_model_config* glc_engine_config(const glc_engine* e);
int glc_engine_dtype(const glc_engine* e);

#ifdef __cplusplus
}
#endif
#endif /* GLICLASS_HIP_H */
