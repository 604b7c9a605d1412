/*
 * Native checkpoint importer: an HF model directory (config.json + model.safetensors) or a
 * .safetensors file with config.json beside it -> glc_weights, so create_ort_session() can open what the reference's
 * launcher downloads (/root/reference/run_GLiClass.sh:34-36) without the ONNX export step
 * (/root/reference/ONNX_CONVERTING/convert_to_onnx.py:48-78).  Pure C: the host layer's JSON reader parses both
 * config.json and the safetensors header (8-byte little-endian length, JSON {"name": {"dtype","shape","data_offsets"}},
 * raw little-endian tensor data); F32 / F16 / BF16 tensors are widened to fp32.
 *
 * Tensor names are HF's (`DebertaV2Model` / `Qwen2Model` / `Qwen3Model` / `LlamaModel` / `ModernBertModel` / `BertModel` / `RobertaModel` / `T5EncoderModel` state_dict) under any of the prefixes GLiClass checkpoints use
 * (the BERT family's query / key / value projections are concatenated into the fused Wqkv of the tensor order, and so are T5's q / k / v and
 * its wi_0 / wi_1; a T5 checkpoint's decoder-side tensors are ignored);
 * configuration fields follow transformers' DebertaV2Config / Qwen2Config inside `encoder_config`, and the GLiClass
 * fields as restated in SURVEY.md §8a row a12 (class_token_index, text_token_index, pooling_strategy, scorer_type,
 * embed_class_token, normalize_features ...).  The GLiClass field names come from the upstream python package, which
 * is not available offline: that part is UNPINNED, so anything the engine does not implement is rejected loudly instead
 * of being guessed (other scorers, LSTM, bi-encoder architectures, conv layer, absolute positions ...).
 */
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "glc_json.h"
#include "glc_weights.h"

static const char* const kPrefixes[] = {"", "model.", "deberta.", "encoder_model.model.", "model.encoder_model.model.",
                                        "encoder_model.", "model.encoder_model.", "decoder_model.model.", "model.decoder_model.model.",
                                        "encoder_model.deberta.", "model.encoder_model.deberta.",
                                        "bert.", "roberta.", "encoder_model.bert.", "encoder_model.roberta.", "model.encoder_model.bert.",
                                        "model.encoder_model.roberta."};
#define N_PREFIXES (sizeof(kPrefixes) / sizeof(kPrefixes[0]))

static double jnum(const gj_value* o, const char* k, double dflt) {
    const gj_value* v = gj_get(o, k);
    return gj_is(v, GJ_NUM) ? v->u.num : dflt;
}
static int jflag(const gj_value* o, const char* k, int dflt) {
    const gj_value* v = gj_get(o, k);
    if (gj_is(v, GJ_BOOL)) return v->u.boolean;
    if (gj_is(v, GJ_NUM)) return v->u.num != 0;
    return dflt;
}
static const char* jtext(const gj_value* o, const char* k) {
    const gj_value* v = gj_get(o, k);
    return gj_is(v, GJ_STR) ? v->u.str.s : NULL;
}
/* "p2c|c2p" or ["p2c","c2p"] */
static int list_has(const gj_value* v, const char* item) {
    if (gj_is(v, GJ_STR)) return strstr(v->u.str.s, item) != NULL;
    if (gj_is(v, GJ_ARR)) for (size_t i = 0; i < v->u.arr.n; ++i) if (gj_is(v->u.arr.items[i], GJ_STR) && !strcmp(v->u.arr.items[i]->u.str.s, item)) return 1;
    return 0;
}

static char* slurp(const char* path, size_t* len) {
    FILE* f = fopen(path, "rb");
    if (!f) return NULL;
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    char* b = (char*)malloc((size_t)(n > 0 ? n : 0) + 1);
    if (!b) { fclose(f); return NULL; }
    size_t got = fread(b, 1, (size_t)(n > 0 ? n : 0), f);
    fclose(f);
    b[got] = 0; *len = got;
    return b;
}

#define REJECT(...) do { fprintf(stderr, "Error: checkpoint config: " __VA_ARGS__); fputc('\n', stderr); return -1; } while (0)

static int parse_config(const gj_value* root, glc_model_config* c) {
    memset(c, 0, sizeof(*c));
    const gj_value* enc = gj_get(root, "encoder_config");
    if (!gj_is(enc, GJ_OBJ)) enc = root;                                  /* a bare backbone config */
    const char* mt = jtext(enc, "model_type");
    if (!mt) REJECT("no model_type");
    /* (a *ForSequenceClassification checkpoint — the block at the end of this function — on a backbone that has no such head here) */
    const gj_value* archs = gj_get(root, "architectures");
    int seqcls = 0;
    if (gj_is(archs, GJ_ARR))
        for (size_t i = 0; i < archs->u.arr.n; ++i) {
            const gj_value* a = archs->u.arr.items[i];
            static const char sfx[] = "ForSequenceClassification";
            if (gj_is(a, GJ_STR) && a->u.str.len >= sizeof sfx - 1 && !strcmp(a->u.str.s + a->u.str.len - (sizeof sfx - 1), sfx)) seqcls = 1;
        }
    if (seqcls && strcmp(mt, "deberta-v2") && strcmp(mt, "bert") && strcmp(mt, "roberta") && strcmp(mt, "xlm-roberta") && strcmp(mt, "modernbert"))
        REJECT("model_type '%s' has no sequence-classification head in this engine (deberta-v2, bert, roberta, xlm-roberta, modernbert; decoder and T5 classes are out of scope)", mt);
    const char* arch = jtext(root, "architecture_type");
    if (arch && strcmp(arch, "uni-encoder")) REJECT("architecture_type '%s' is not implemented (only uni-encoder)", arch);
    if (jflag(root, "use_lstm", 0)) REJECT("use_lstm=true is not implemented");
    const char* scorer = jtext(root, "scorer_type");
    int scorer_id = GLC_SCORER_DOT;
    if (scorer) {
        if (!strcmp(scorer, "simple")) scorer_id = GLC_SCORER_DOT;
        else if (!strcmp(scorer, "weighted-dot")) scorer_id = GLC_SCORER_WEIGHTED_DOT;
        else if (!strcmp(scorer, "mlp")) scorer_id = GLC_SCORER_MLP;
        else REJECT("scorer_type '%s' is not implemented (simple, weighted-dot, mlp)", scorer);
    }
    const char* pool = jtext(root, "pooling_strategy");
    c->pooling = GLC_POOL_FIRST;
    if (pool) {
        if (!strcmp(pool, "first")) c->pooling = GLC_POOL_FIRST;
        else if (!strcmp(pool, "avg")) c->pooling = GLC_POOL_AVG;
        else if (!strcmp(pool, "last")) c->pooling = GLC_POOL_LAST;
        else REJECT("pooling_strategy '%s' is not implemented (first, avg, last)", pool);
    }
    c->scorer = scorer_id;
    c->embed_class_token = jflag(root, "embed_class_token", 1);
    c->normalize_features = jflag(root, "normalize_features", 0);
    c->logit_scale = (float)jnum(root, "logit_scale", 1.0);
    c->class_token_index = (int32_t)jnum(root, "class_token_index", -1);
    c->text_token_index = (int32_t)jnum(root, "text_token_index", -1);
    c->pad_id = (int32_t)jnum(enc, "pad_token_id", 0);
    c->cls_id = (int32_t)jnum(enc, "cls_token_id", jnum(enc, "bos_token_id", 1));
    c->sep_id = (int32_t)jnum(enc, "sep_token_id", jnum(enc, "eos_token_id", 2));
    const int is_t5 = !strcmp(mt, "t5") || !strcmp(mt, "mt5");          /* T5Config names its dimensions d_model / num_layers / num_heads / d_ff / d_kv */
    if (!strcmp(mt, "umt5")) REJECT("model_type 'umt5' is not implemented (a relative_attention_bias table per layer; t5 and mt5 share layer 0's)");
    c->hidden = (int32_t)jnum(enc, is_t5 ? "d_model" : "hidden_size", 0);
    c->layers = (int32_t)jnum(enc, is_t5 ? "num_layers" : "num_hidden_layers", 0);
    c->heads = (int32_t)jnum(enc, is_t5 ? "num_heads" : "num_attention_heads", 0);
    c->inter = (int32_t)jnum(enc, is_t5 ? "d_ff" : "intermediate_size", 0);
    c->vocab = (int32_t)jnum(root, "vocab_size", jnum(enc, "vocab_size", 0));
    if (c->hidden <= 0 || c->layers <= 0 || c->heads <= 0 || c->inter <= 0 || (!is_t5 && c->hidden % c->heads)) REJECT("missing or inconsistent backbone dimensions");
    c->head_dim = is_t5 ? (int32_t)jnum(enc, "d_kv", 64) : c->hidden / c->heads;
    c->qk_norm = 0; c->attn_bias = 1;
    if (!strcmp(mt, "deberta-v2")) {
        c->backbone = GLC_BACKBONE_DEBERTA;
        c->kv_heads = c->heads; c->causal = 1; c->rope_theta = 1.0e6f;   /* unused by this backbone; the blob header's defaults */
        c->ln_eps = (float)jnum(enc, "layer_norm_eps", 1e-7);
        if (!jflag(enc, "relative_attention", 0)) REJECT("relative_attention=false is not implemented");
        const gj_value* pat = gj_get(enc, "pos_att_type");
        if (!list_has(pat, "c2p") || !list_has(pat, "p2c")) REJECT("pos_att_type must contain c2p and p2c");
        if (!jflag(enc, "share_att_key", 0)) REJECT("share_att_key=false is not implemented");
        const char* nre = jtext(enc, "norm_rel_ebd");
        if (!nre || !strstr(nre, "layer_norm")) REJECT("norm_rel_ebd must be layer_norm");
        if (jflag(enc, "position_biased_input", 1)) REJECT("position_biased_input=true is not implemented");
        if (jnum(enc, "type_vocab_size", 0) != 0) REJECT("type_vocab_size != 0 is not implemented");
        if (jnum(enc, "conv_kernel_size", 0) > 0) REJECT("conv_kernel_size > 0 (ConvLayer) is not implemented");
        int mrp = (int)jnum(enc, "max_relative_positions", -1);
        if (mrp < 1) mrp = (int)jnum(enc, "max_position_embeddings", 512);        /* modeling_deberta_v2.py:586-588 */
        c->max_rel_pos = mrp;
        c->pos_buckets = (int32_t)jnum(enc, "position_buckets", -1);
        if (c->pos_buckets < 1) c->pos_buckets = 0;
    } else if (!strcmp(mt, "qwen2")) {
        c->backbone = GLC_BACKBONE_DECODER;
        c->kv_heads = (int32_t)jnum(enc, "num_key_value_heads", c->heads);
        c->causal = jflag(root, "causal", 1);                                      /* BASELINE.json: causal; upstream wrapping unpinned */
        c->ln_eps = (float)jnum(enc, "rms_norm_eps", 1e-6);
        c->rope_theta = (float)jnum(enc, "rope_theta", 1.0e6);
        c->pos_buckets = 0; c->max_rel_pos = 0;
        if (!pool) c->pooling = GLC_POOL_LAST;
        if (c->kv_heads <= 0 || c->heads % c->kv_heads) REJECT("num_key_value_heads does not divide num_attention_heads");
    } else if (!strcmp(mt, "qwen3") || !strcmp(mt, "llama")) {
        /* transformers models/qwen3 (per-head RMSNorm on Q and K before RoPE, its own head_dim) and models/llama: the Qwen2 stack without
         * (or, attention_bias: true, with) the q / k / v biases.  Anything that changes the arithmetic beyond that is refused by name. */
        c->backbone = GLC_BACKBONE_DECODER;
        c->qk_norm = !strcmp(mt, "qwen3");
        c->attn_bias = jflag(enc, "attention_bias", 0);
        c->head_dim = (int32_t)jnum(enc, "head_dim", (double)(c->hidden / c->heads));
        c->kv_heads = (int32_t)jnum(enc, "num_key_value_heads", c->heads);
        c->causal = jflag(root, "causal", 1);
        c->ln_eps = (float)jnum(enc, "rms_norm_eps", 1e-6);
        c->rope_theta = (float)jnum(enc, "rope_theta", c->qk_norm ? 1.0e6 : 1.0e4);
        c->pos_buckets = 0; c->max_rel_pos = 0;
        if (!pool) c->pooling = GLC_POOL_LAST;
        if (c->kv_heads <= 0 || c->heads % c->kv_heads) REJECT("num_key_value_heads does not divide num_attention_heads");
        if (c->head_dim != 64 && c->head_dim != 128) REJECT("head_dim %d is not implemented (64, 128)", c->head_dim);
        if (jflag(enc, "mlp_bias", 0)) REJECT("mlp_bias=true is not implemented");
        if (jflag(enc, "use_sliding_window", 0)) REJECT("use_sliding_window=true is not implemented");
        const gj_value* lt = gj_get(enc, "layer_types");
        if (gj_is(lt, GJ_ARR) && list_has(lt, "sliding_attention")) REJECT("layer_types with a 'sliding_attention' entry is not implemented");
        const char* act = jtext(enc, "hidden_act");
        if (act && strcmp(act, "silu")) REJECT("hidden_act '%s' is not implemented (silu)", act);
        /* RoPE: the default rotation only (Llama-3.x frequency scaling, linear / dynamic / yarn are out of scope).  transformers 4 writes
         * rope_scaling {rope_type | type}, transformers 5 rope_parameters {rope_type, rope_theta}. */
        static const char* const rk[2] = {"rope_scaling", "rope_parameters"};
        for (int q = 0; q < 2; ++q) {
            const gj_value* rs = gj_get(enc, rk[q]);
            if (!gj_is(rs, GJ_OBJ)) continue;
            const char* rt = jtext(rs, "rope_type");
            if (!rt) rt = jtext(rs, "type");
            if (rt && strcmp(rt, "default")) REJECT("%s type '%s' is not implemented (default)", rk[q], rt);
            c->rope_theta = (float)jnum(rs, "rope_theta", c->rope_theta);
        }
    } else if (!strcmp(mt, "modernbert")) {
        /* transformers models/modernbert: configuration_modernbert.py (both the transformers-5 form with layer_types / rope_parameters
         * and the older one with global_attn_every_n_layers / global_rope_theta / local_rope_theta) */
        c->backbone = GLC_BACKBONE_MODERNBERT;
        c->kv_heads = c->heads; c->causal = 0;
        c->pos_buckets = 0; c->max_rel_pos = 0;
        c->ln_eps = (float)jnum(enc, "norm_eps", 1e-5);
        if (jflag(enc, "attention_bias", 0)) REJECT("attention_bias=true is not implemented");
        if (jflag(enc, "mlp_bias", 0)) REJECT("mlp_bias=true is not implemented");
        if (jflag(enc, "norm_bias", 0)) REJECT("norm_bias=true is not implemented");
        const char* act = jtext(enc, "hidden_activation");
        if (act && strcmp(act, "gelu")) REJECT("hidden_activation '%s' is not implemented (gelu)", act);
        if (c->head_dim != 64) REJECT("head_dim %d is not implemented (64)", c->head_dim);
        const int la = (int)jnum(enc, "local_attention", 128);
        if (la < 0 || la % 2) REJECT("local_attention %d is not implemented (an even window)", la);
        c->local_window = la / 2;
        int every = (int)jnum(enc, "global_attn_every_n_layers", 3);
        const gj_value* lt = gj_get(enc, "layer_types");
        if (gj_is(lt, GJ_ARR)) {
            /* a list of the periodic form: full on l % every == 0, sliding elsewhere; its period is the first sliding layer's distance
             * to the full layer before it (or "all full") */
            if ((int)lt->u.arr.n != c->layers) REJECT("layer_types has %zu entries for %d layers", lt->u.arr.n, c->layers);
            every = c->layers > 0 ? c->layers : 1;
            for (int l = 0; l < c->layers; ++l) {
                const gj_value* v = lt->u.arr.items[l];
                if (!gj_is(v, GJ_STR) || (strcmp(v->u.str.s, "full_attention") && strcmp(v->u.str.s, "sliding_attention")))
                    REJECT("layer_types[%d] is not 'full_attention' or 'sliding_attention'", l);
                if (l > 0 && !strcmp(v->u.str.s, "full_attention") && every == c->layers) { every = l; break; }
            }
            for (int l = 0; l < c->layers; ++l)
                if ((strcmp(lt->u.arr.items[l]->u.str.s, "full_attention") == 0) != (l % every == 0))
                    REJECT("layer_types is not periodic (full attention on every n-th layer from layer 0)");
        }
        if (every < 1) REJECT("global_attn_every_n_layers must be positive");
        c->global_every = every;
        c->rope_theta = (float)jnum(enc, "global_rope_theta", 160000.0);
        c->rope_theta_local = (float)jnum(enc, "local_rope_theta", 10000.0);
        const gj_value* rp = gj_get(enc, "rope_parameters");
        if (gj_is(rp, GJ_OBJ)) {
            const gj_value* fa = gj_get(rp, "full_attention");
            const gj_value* sa = gj_get(rp, "sliding_attention");
            if (gj_is(fa, GJ_OBJ)) c->rope_theta = (float)jnum(fa, "rope_theta", c->rope_theta);
            if (gj_is(sa, GJ_OBJ)) c->rope_theta_local = (float)jnum(sa, "rope_theta", c->rope_theta_local);
            const char* rt = gj_is(fa, GJ_OBJ) ? jtext(fa, "rope_type") : NULL;
            const char* rs = gj_is(sa, GJ_OBJ) ? jtext(sa, "rope_type") : NULL;
            if ((rt && strcmp(rt, "default")) || (rs && strcmp(rs, "default"))) REJECT("rope_type other than 'default' is not implemented");
        }
    } else if (!strcmp(mt, "bert") || !strcmp(mt, "roberta") || !strcmp(mt, "xlm-roberta")) {
        /* transformers models/bert, models/roberta, models/xlm_roberta: one arithmetic; RoBERTa / XLM-R number the non-pad tokens from
         * pad_token_id + 1 on (create_position_ids_from_input_ids), BERT numbers the positions from 0 */
        const int is_bert = !strcmp(mt, "bert");
        c->backbone = GLC_BACKBONE_BERT;
        c->kv_heads = c->heads; c->causal = 0; c->rope_theta = 1.0e6f; c->global_every = 1; c->rope_theta_local = 1.0e4f;
        c->pos_buckets = 0; c->max_rel_pos = 0;
        c->ln_eps = (float)jnum(enc, "layer_norm_eps", 1e-12);
        c->pad_id = (int32_t)jnum(enc, "pad_token_id", is_bert ? 0 : 1);
        const char* pet = jtext(enc, "position_embedding_type");
        if (pet && strcmp(pet, "absolute")) REJECT("position_embedding_type '%s' is not implemented (absolute)", pet);
        const char* act = jtext(enc, "hidden_act");
        if (act && strcmp(act, "gelu")) REJECT("hidden_act '%s' is not implemented (gelu)", act);
        if (jflag(enc, "is_decoder", 0)) REJECT("is_decoder=true is not implemented");
        if (jflag(enc, "add_cross_attention", 0)) REJECT("add_cross_attention=true is not implemented");
        if (c->head_dim != 64) REJECT("head_dim %d is not implemented (64)", c->head_dim);
        c->pos_offset = is_bert ? 0 : c->pad_id + 1;
        c->max_positions = (int32_t)jnum(enc, "max_position_embeddings", 512);
        c->type_vocab = (int32_t)jnum(enc, "type_vocab_size", 2);
        if (c->pad_id < 0) REJECT("pad_token_id %d is negative", c->pad_id);
        if (c->max_positions - c->pos_offset < 1) REJECT("max_position_embeddings %d leaves no position behind the offset %d", c->max_positions, c->pos_offset);
        if (c->type_vocab < 1) REJECT("type_vocab_size %d is not implemented (at least 1)", c->type_vocab);
    } else if (is_t5) {
        /* transformers models/t5 (T5 v1.1, mT5, flan-T5 through T5EncoderModel): the encoder stack only */
        c->backbone = GLC_BACKBONE_T5;
        c->kv_heads = c->heads; c->causal = 0; c->rope_theta = 1.0e6f; c->global_every = 1; c->rope_theta_local = 1.0e4f;
        c->pos_buckets = 0; c->max_rel_pos = 0;
        c->ln_eps = (float)jnum(enc, "layer_norm_epsilon", 1e-6);
        const char* ffp = jtext(enc, "feed_forward_proj");
        if (!ffp) ffp = "relu";
        if (strcmp(ffp, "gated-gelu")) REJECT("feed_forward_proj '%s' is not implemented (gated-gelu)", ffp);
        const char* act = jtext(enc, "dense_act_fn");
        if (act && strcmp(act, "gelu_new")) REJECT("dense_act_fn '%s' is not implemented (gelu_new)", act);
        if (c->head_dim != 64) REJECT("d_kv %d is not implemented (64)", c->head_dim);
        if (jflag(enc, "is_decoder", 0)) REJECT("is_decoder=true is not implemented");
        c->rel_buckets = (int32_t)jnum(enc, "relative_attention_num_buckets", 32);
        c->rel_max_distance = (int32_t)jnum(enc, "relative_attention_max_distance", 128);
        if (c->rel_buckets < 4 || c->rel_buckets % 4 || c->rel_max_distance <= c->rel_buckets / 4)
            REJECT("relative_attention_num_buckets %d / relative_attention_max_distance %d is not implemented (a multiple of 4, max distance beyond a quarter of it)",
                   c->rel_buckets, c->rel_max_distance);
        if (c->pad_id < 0) REJECT("pad_token_id %d is negative", c->pad_id);
    } else REJECT("backbone model_type '%s' is not implemented (deberta-v2, qwen2, qwen3, llama, modernbert, bert, roberta, xlm-roberta, t5, mt5)", mt);
    /* A checkpoint saved by an HF *ForSequenceClassification class (`architectures` names it; a bare HF config, no GLiClass wrapper keys):
     * the sequence-classification head (head_kind = GLC_HEAD_SEQCLS, include/gliclass_hip.h) behind the backbone parsed above.  Mirrors
     * seqcls_config_from_hf of gliclass/c_amd/weights.py; the head arithmetic per class and its transformers sources: csrc/cls_head.hip. */
    if (seqcls) {
        const gj_value* i2l = gj_get(root, "id2label");
        const int K = gj_is(i2l, GJ_OBJ) && i2l->u.obj.n > 0 ? (int)i2l->u.obj.n : (int)jnum(root, "num_labels", 2);
        if (K < 1 || K > GLC_CLS_MAX_LABELS) REJECT("num_labels %d is not implemented (1 .. %d)", K, GLC_CLS_MAX_LABELS);
        c->head_kind = GLC_HEAD_SEQCLS; c->cls_labels = K; c->cls_dense = 1; c->cls_norm = 0; c->pooling = GLC_POOL_FIRST;
        c->scorer = GLC_SCORER_DOT;
        if (c->backbone == GLC_BACKBONE_BERT) c->cls_act = GLC_CLS_ACT_TANH;                 /* BertPooler / RobertaClassificationHead */
        else if (c->backbone == GLC_BACKBONE_MODERNBERT) {                                   /* ModernBertPredictionHead */
            const char* act = jtext(root, "classifier_activation");
            if (act && strcmp(act, "gelu")) REJECT("classifier_activation '%s' is not implemented (gelu)", act);
            const char* cp = jtext(root, "classifier_pooling");
            if (cp && strcmp(cp, "cls") && strcmp(cp, "mean")) REJECT("classifier_pooling '%s' is not implemented (cls, mean)", cp);
            c->pooling = cp && !strcmp(cp, "mean") ? GLC_POOL_AVG : GLC_POOL_FIRST;
            c->cls_act = GLC_CLS_ACT_GELU; c->cls_norm = 1;
        } else {                                                                             /* DeBERTa ContextPooler */
            const int phs = (int)jnum(root, "pooler_hidden_size", (double)c->hidden);
            if (phs != c->hidden) REJECT("pooler_hidden_size %d != hidden_size %d is not implemented", phs, c->hidden);
            const char* act = jtext(root, "pooler_hidden_act");
            if (act && strcmp(act, "gelu")) REJECT("pooler_hidden_act '%s' is not implemented (gelu)", act);
            c->cls_act = GLC_CLS_ACT_GELU;
        }
    }
    return 0;
}

/* checkpoint name of slot k of the sequence-classification head (include/gliclass_hip.h order) for the class the config names; NULL: the class
 * has no such tensor.  Looked up under the importer's prefixes ("" and "bert." among them: DeBERTa's pooler sits at the top level, BERT's
 * inside the backbone). */
static const char* cls_head_key(const glc_model_config* c, int k) {
    static const char* const pooler[6] = {"pooler.dense.weight", "pooler.dense.bias", NULL, NULL, "classifier.weight", "classifier.bias"};
    static const char* const roberta[6] = {"classifier.dense.weight", "classifier.dense.bias", NULL, NULL, "classifier.out_proj.weight", "classifier.out_proj.bias"};
    static const char* const mbert[6] = {"head.dense.weight", "head.dense.bias", "head.norm.weight", "head.norm.bias", "classifier.weight", "classifier.bias"};
    if (k < 0 || k >= GLC_TENSORS_CLS_HEAD) return NULL;
    if (c->backbone == GLC_BACKBONE_MODERNBERT) return mbert[k];
    if (c->backbone == GLC_BACKBONE_BERT && c->pos_offset != 0) return roberta[k];           /* RoBERTa / XLM-R (BERT numbers positions from 0) */
    return pooler[k];
}

typedef struct { const gj_value* hdr; const unsigned char* data; size_t data_len; } st_file;

static const gj_value* st_find(const st_file* st, const char* name, char* found, size_t fcap) {
    for (size_t p = 0; p < N_PREFIXES; ++p) {
        snprintf(found, fcap, "%s%s", kPrefixes[p], name);
        const gj_value* v = gj_get(st->hdr, found);
        if (gj_is(v, GJ_OBJ)) return v;
    }
    return NULL;
}

static float half_to_float(uint16_t h) {
    uint32_t sign = (uint32_t)(h & 0x8000u) << 16, exp = (h >> 10) & 0x1Fu, man = h & 0x3FFu, bits;
    if (exp == 0) {
        if (!man) bits = sign;
        else { int e = -1; do { man <<= 1; ++e; } while (!(man & 0x400u)); bits = sign | ((uint32_t)(127 - 15 - e) << 23) | ((man & 0x3FFu) << 13); }
    } else if (exp == 31) bits = sign | 0x7F800000u | (man << 13);
    else bits = sign | ((exp + 112u) << 23) | (man << 13);
    float f; memcpy(&f, &bits, 4); return f;
}

/* tensor `name` (under any known prefix) with the shape shp[0 .. nd) -> n fp32 values at dst; F32 / F16 / BF16 are read.  0, or -1 with a message */
static int st_read_f32(const st_file* st, const char* stp, const char* name, int nd, const uint64_t* shp, float* dst) {
    char found[200];
    const size_t n = (size_t)shp[0] * (nd > 1 ? (size_t)shp[1] : 1);
    const gj_value* t = st_find(st, name, found, sizeof found);
    if (!t) { fprintf(stderr, "Error: '%s': tensor '%s' not found under any known prefix\n", stp, name); return -1; }
    const char* dt = jtext(t, "dtype");
    const gj_value* shape = gj_get(t, "shape");
    const gj_value* offs = gj_get(t, "data_offsets");
    if (!dt || !gj_is(shape, GJ_ARR) || !gj_is(offs, GJ_ARR) || offs->u.arr.n != 2) { fprintf(stderr, "Error: '%s': malformed entry '%s'\n", stp, found); return -1; }
    int shape_ok = (int)shape->u.arr.n == nd;
    for (int d = 0; shape_ok && d < nd; ++d) shape_ok = (uint64_t)shape->u.arr.items[d]->u.num == shp[d];
    if (!shape_ok) { fprintf(stderr, "Error: '%s': tensor '%s' has an unexpected shape (want %llu x %llu)\n", stp, found, (unsigned long long)shp[0], (unsigned long long)(nd > 1 ? shp[1] : 1)); return -1; }
    size_t b0 = (size_t)offs->u.arr.items[0]->u.num, b1 = (size_t)offs->u.arr.items[1]->u.num;
    size_t esz = !strcmp(dt, "F32") ? 4 : (!strcmp(dt, "F16") || !strcmp(dt, "BF16")) ? 2 : 0;
    if (!esz) { fprintf(stderr, "Error: '%s': tensor '%s' has dtype %s (F32, F16, BF16 are read)\n", stp, found, dt); return -1; }
    if (b1 < b0 || b1 > st->data_len || b1 - b0 != n * esz) { fprintf(stderr, "Error: '%s': tensor '%s' has bad data offsets\n", stp, found); return -1; }
    const unsigned char* src = st->data + b0;
    if (esz == 4) memcpy(dst, src, n * 4);
    else if (dt[0] == 'B') for (size_t k = 0; k < n; ++k) { uint32_t u = ((uint32_t)src[2 * k] | ((uint32_t)src[2 * k + 1] << 8)) << 16; memcpy(&dst[k], &u, 4); }
    else for (size_t k = 0; k < n; ++k) dst[k] = half_to_float((uint16_t)(src[2 * k] | (src[2 * k + 1] << 8)));
    return 0;
}

int glc_load_hf_checkpoint(const char* path, glc_weights* w) {
    char dir[3072], stp[4096], cfp[4096], err[200];
    struct stat sb;
    if (stat(path, &sb) != 0) { fprintf(stderr, "Error: cannot open model '%s'\n", path); return -1; }
    if (S_ISDIR(sb.st_mode)) snprintf(dir, sizeof dir, "%s", path);
    else {
        snprintf(dir, sizeof dir, "%s", path);
        char* slash = strrchr(dir, '/');
        if (slash) *slash = 0; else snprintf(dir, sizeof dir, ".");
    }
    if (S_ISDIR(sb.st_mode)) snprintf(stp, sizeof stp, "%s/model.safetensors", dir); else snprintf(stp, sizeof stp, "%s", path);
    snprintf(cfp, sizeof cfp, "%s/config.json", dir);

    size_t clen = 0;
    char* ctext = slurp(cfp, &clen);
    if (!ctext) { fprintf(stderr, "Error: cannot read '%s'\n", cfp); return -1; }
    gj_doc* cdoc = gj_parse(ctext, clen, 0, err, sizeof err);
    free(ctext);
    if (!cdoc) { fprintf(stderr, "Error: %s: %s\n", cfp, err); return -1; }
    int rc = parse_config(gj_root(cdoc), &w->cfg);
    gj_free(cdoc);
    if (rc) return -1;

    int fd = open(stp, O_RDONLY);
    if (fd < 0) {
        char idx[4200]; snprintf(idx, sizeof idx, "%s/model.safetensors.index.json", dir);
        if (access(idx, R_OK) == 0) fprintf(stderr, "Error: '%s' is a sharded checkpoint; merge it into one model.safetensors first\n", dir);
        else fprintf(stderr, "Error: cannot open '%s'\n", stp);
        return -1;
    }
    if (fstat(fd, &sb) != 0 || sb.st_size < 8) { close(fd); fprintf(stderr, "Error: '%s' is not a safetensors file\n", stp); return -1; }
    void* m = mmap(NULL, (size_t)sb.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (m == MAP_FAILED) { fprintf(stderr, "Error: mmap of '%s' failed\n", stp); return -1; }
    const unsigned char* b = (const unsigned char*)m;
    uint64_t hlen = 0;
    for (int i = 7; i >= 0; --i) hlen = (hlen << 8) | b[i];
    gj_doc* hdoc = NULL;
    rc = -1;
    if (hlen > (uint64_t)sb.st_size - 8) { fprintf(stderr, "Error: '%s': header length beyond the file\n", stp); goto done; }
    hdoc = gj_parse((const char*)b + 8, (size_t)hlen, 0, err, sizeof err);
    if (!hdoc || !gj_is(gj_root(hdoc), GJ_OBJ)) { fprintf(stderr, "Error: '%s': %s\n", stp, hdoc ? "header is not an object" : err); goto done; }
    st_file st = {gj_root(hdoc), b + 8 + hlen, (size_t)sb.st_size - 8 - (size_t)hlen};

    glc_model_config* c = &w->cfg;
    char found[200];
    /* the embedding matrix decides the vocabulary size (tokens were added after the backbone config was written) */
    const gj_value* emb = st_find(&st, c->backbone == GLC_BACKBONE_DECODER ? "embed_tokens.weight" : c->backbone == GLC_BACKBONE_T5 ? "shared.weight" :
                                       c->backbone == GLC_BACKBONE_MODERNBERT ? "embeddings.tok_embeddings.weight" : "embeddings.word_embeddings.weight", found, sizeof found);
    const char* t5_emb = "shared.weight";                 /* (a bare T5EncoderModel may store the tied copy only) */
    if (c->backbone == GLC_BACKBONE_T5 && !emb) { t5_emb = "encoder.embed_tokens.weight"; emb = st_find(&st, t5_emb, found, sizeof found); }
    if (c->backbone == GLC_BACKBONE_T5 && !st_find(&st, "encoder.block.0.layer.0.SelfAttention.q.weight", found, sizeof found)) {
        fprintf(stderr, "Error: '%s': is_encoder_decoder: the checkpoint holds no encoder tensors (encoder.block.0.layer.0.SelfAttention.q.weight)\n", stp); goto done;
    }
    const gj_value* eshape = gj_get(emb, "shape");
    if (!emb || !gj_is(eshape, GJ_ARR) || eshape->u.arr.n != 2) { fprintf(stderr, "Error: '%s': no word-embedding tensor under any known prefix\n", stp); goto done; }
    c->vocab = (int32_t)eshape->u.arr.items[0]->u.num;
    if (c->class_token_index < 0) c->class_token_index = c->vocab - 2;
    if (c->text_token_index < 0) c->text_token_index = c->vocab - 1;

    if (c->backbone == GLC_BACKBONE_DECODER) {
        /* q_norm / k_norm exactly when the configuration says so: a checkpoint that carries gains the forward would not apply (or lacks
         * the ones it would) is another model than its config.json names */
        static const char* const qk[2] = {"layers.0.self_attn.q_norm.weight", "layers.0.self_attn.k_norm.weight"};
        for (int q = 0; q < 2; ++q) {
            const int have = st_find(&st, qk[q], found, sizeof found) != NULL;
            if (have && !c->qk_norm) { fprintf(stderr, "Error: '%s': tensor '%s' is present, but this model_type has no q_norm / k_norm\n", stp, found); goto done; }
            if (!have && c->qk_norm) { fprintf(stderr, "Error: '%s': tensor '%s' is missing (model_type qwen3 needs q_norm and k_norm)\n", stp, qk[q]); goto done; }
        }
        /* (Llama / Qwen3 with attention_bias: true give o_proj a bias as well; the tensor order has no slot for it) */
        if (st_find(&st, "layers.0.self_attn.o_proj.bias", found, sizeof found)) { fprintf(stderr, "Error: '%s': tensor '%s' (an output-projection bias) is not implemented\n", stp, found); goto done; }
    }
    w->n_tensors = glc_num_tensors_cfg(c);
    w->tensors = (const float**)calloc((size_t)w->n_tensors, sizeof(float*));
    if (!w->tensors) goto done;
    char tn[96]; uint64_t shp[4]; double amp, mean; size_t total = 0;
    for (int i = 0; i < w->n_tensors; ++i) {
        int nd = glc_tensor_spec(c, i, tn, shp, &amp, &mean);
        if (nd < 0) goto done;
        total += ((size_t)shp[0] * (nd > 1 ? (size_t)shp[1] : 1) + 15) / 16 * 16;
    }
    w->_owned = (float*)malloc(total * sizeof(float));
    if (!w->_owned) { fprintf(stderr, "Error: cannot allocate %zu bytes for the checkpoint\n", total * sizeof(float)); goto done; }
    size_t off = 0;
    for (int i = 0; i < w->n_tensors; ++i) {
        int nd = glc_tensor_spec(c, i, tn, shp, &amp, &mean);
        size_t n = (size_t)shp[0] * (nd > 1 ? (size_t)shp[1] : 1);
        /* sequence-classification head: the class's own names; a bias the checkpoint has switched off (ModernBERT classifier_bias /
         * norm_bias = false) and a stage the class does not have stay NULL (glc_engine_create decides which slots may be empty) */
        if (c->head_kind == GLC_HEAD_SEQCLS && i >= w->n_tensors - GLC_TENSORS_CLS_HEAD) {
            const int k = i - (w->n_tensors - GLC_TENSORS_CLS_HEAD);
            const char* key = cls_head_key(c, k);
            const int optional = k == 1 || k == 3 || k == 5;
            if (!key || (optional && !st_find(&st, key, found, sizeof found))) continue;
            if (st_read_f32(&st, stp, key, nd, shp, w->_owned + off)) goto done;
            w->tensors[i] = w->_owned + off;
            off += (n + 15) / 16 * 16;
            continue;
        }
        /* BERT family: the fused Wqkv rows (and bias) are the checkpoint's query | key | value tensors, one after the other */
        const char* fq = c->backbone == GLC_BACKBONE_BERT ? strstr(tn, ".attention.self.Wqkv.") : NULL;
        if (fq) {
            static const char* const part[3] = {"query", "key", "value"};
            const uint64_t prow = shp[0] / 3;
            int bad = 0;
            for (int q = 0; q < 3 && !bad; ++q) {
                char pn[128];
                snprintf(pn, sizeof pn, "%.*s.attention.self.%s.%s", (int)(fq - tn), tn, part[q], fq + strlen(".attention.self.Wqkv."));
                uint64_t pshp[2] = {prow, nd > 1 ? shp[1] : 0};
                if (st_read_f32(&st, stp, pn, nd, pshp, w->_owned + off + (size_t)q * (n / 3))) bad = 1;
            }
            if (bad) goto done;
            w->tensors[i] = w->_owned + off;
            off += (n + 15) / 16 * 16;
            continue;
        }
        /* T5: the fused Wqkv rows are the checkpoint's q | k | v, the fused Wgu rows its wi_0 | wi_1 */
        const char* tq = c->backbone == GLC_BACKBONE_T5 ? strstr(tn, ".SelfAttention.Wqkv.") : NULL;
        const char* tg = c->backbone == GLC_BACKBONE_T5 ? strstr(tn, ".DenseReluDense.Wgu.") : NULL;
        if (tq || tg) {
            static const char* const qkv[3] = {"q", "k", "v"};
            static const char* const gu[2] = {"wi_0", "wi_1"};
            const int np = tq ? 3 : 2;
            const char* at = tq ? tq : tg;
            const size_t skip = strlen(tq ? ".SelfAttention.Wqkv." : ".DenseReluDense.Wgu.");
            int bad = 0;
            for (int q = 0; q < np && !bad; ++q) {
                char pn[160];
                snprintf(pn, sizeof pn, "%.*s.%s.%s.%s", (int)(at - tn), tn, tq ? "SelfAttention" : "DenseReluDense", tq ? qkv[q] : gu[q], at + skip);
                uint64_t pshp[2] = {shp[0] / (uint64_t)np, shp[1]};
                if (st_read_f32(&st, stp, pn, nd, pshp, w->_owned + off + (size_t)q * (n / (size_t)np))) bad = 1;
            }
            if (bad) goto done;
            w->tensors[i] = w->_owned + off;
            off += (n + 15) / 16 * 16;
            continue;
        }
        if (st_read_f32(&st, stp, (c->backbone == GLC_BACKBONE_T5 && i == 0) ? t5_emb : tn, nd, shp, w->_owned + off)) goto done;
        w->tensors[i] = w->_owned + off;
        off += (n + 15) / 16 * 16;
    }
    rc = 0;
done:
    if (hdoc) gj_free(hdoc);
    munmap(m, (size_t)sb.st_size);
    return rc;
}
