// The sequence-classification head (head_kind = GLC_HEAD_SEQCLS, include/gliclass_hip.h) behind the pooled-row gather, and the zero-shot NLI
// reduction over its logits.  One parametrisation (cls_dense, cls_act, cls_norm, pooling) covers the four heads of the installed transformers:
//
//   DebertaV2ForSequenceClassification (models/deberta_v2/modeling_deberta_v2.py): ContextPooler.forward — context_token = hidden_states[:, 0];
//     pooled_output = self.dense(context_token); pooled_output = ACT2FN[self.config.pooler_hidden_act](pooled_output) — then
//     logits = self.classifier(pooled_output) (dropout is the identity in eval).                              dense, GELU (erf), no norm, 'first'
//   BertForSequenceClassification (models/bert/modeling_bert.py): BertPooler.forward — first_token_tensor = hidden_states[:, 0];
//     pooled_output = self.dense(first_token_tensor); pooled_output = self.activation(pooled_output) (nn.Tanh) — then
//     logits = self.classifier(pooled_output).                                                                dense, tanh, no norm, 'first'
//   RobertaForSequenceClassification / XLMRobertaForSequenceClassification (models/roberta/modeling_roberta.py, models/xlm_roberta/...):
//     RobertaClassificationHead.forward — x = features[:, 0, :]; x = self.dense(x); x = torch.tanh(x); x = self.out_proj(x).
//                                                                                                             dense, tanh, no norm, 'first'
//   ModernBertForSequenceClassification (models/modernbert/modeling_modernbert.py): classifier_pooling "cls": last_hidden_state[:, 0]; "mean":
//     (last_hidden_state * attention_mask.unsqueeze(-1)).sum(dim=1) / attention_mask.sum(dim=1, keepdim=True); then ModernBertPredictionHead.forward
//     — self.norm(self.act(self.dense(hidden_states))) (Linear with classifier_bias, ACT2FN[classifier_activation], LayerNorm with norm_eps and
//     norm_bias) — and logits = self.classifier(pooled_output).                                               dense, GELU (erf), norm, 'first' / 'avg'
//
// The dense stage is a GEMM of the engine (the split-f16 fp32 path the GLiClass projectors take); everything behind it is ONE launch of the
// row kernel below.  All arithmetic is fp32 in every engine dtype.
#include "glc_common.h"
#include "glc_kernels.h"

namespace {

constexpr int CLS_MAXC = 8;      // chunks of 16 B per lane: H <= 64 * CLS_MAXC * 4 = 2048

// One wave per pooled row: x = act(X[row]) [-> LayerNorm(x) gamma + beta] held in registers, then K dot products against the rows of
// classifier.weight (every wave reads all of it: K H floats, served by L2 after the first wave) reduced with wave shuffles.
__global__ __launch_bounds__(256) void cls_head_kernel(const float* __restrict__ X, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const float* __restrict__ Wc, const float* __restrict__ bc, float* __restrict__ logits,
                                                       int B, int H, int K, int act, float eps) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B) return;                                   // (a whole wave leaves: the shuffles below always see 64 lanes)
    const int lane = threadIdx.x & 63, nch = H >> 2;
    const float* x = X + (size_t)row * H;
    float v[CLS_MAXC][4];
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < CLS_MAXC; ++c) {
        const int ch = lane + 64 * c;
        if (ch < nch) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(x + (size_t)ch * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float a = t[e];
                if (act == 1) a = tanhf(a);
                else if (act == 2) a = glc_gelu(a);
                v[c][e] = a;
                s += a;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[c][e] = 0.f;
        }
    }
    if (gamma) {                                            // torch.nn.LayerNorm: biased variance, two passes over the registers
        const float mean = wave_sum(s) / (float)H;
        float ss = 0.f;
#pragma unroll
        for (int c = 0; c < CLS_MAXC; ++c) {
            if (lane + 64 * c < nch) {
#pragma unroll
                for (int e = 0; e < 4; ++e) { const float d = v[c][e] - mean; ss += d * d; }
            }
        }
        const float rstd = rsqrtf(wave_sum(ss) / (float)H + eps);
#pragma unroll
        for (int c = 0; c < CLS_MAXC; ++c) {
            const int ch = lane + 64 * c;
            if (ch < nch) {
                const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + (size_t)ch * 4);
                f32x4 b = {0.f, 0.f, 0.f, 0.f};
                if (beta) b = *reinterpret_cast<const f32x4*>(beta + (size_t)ch * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[c][e] = (v[c][e] - mean) * rstd * g[e] + b[e];
            }
        }
    }
    for (int k = 0; k < K; ++k) {
        const float* w = Wc + (size_t)k * H;
        float a = 0.f;
#pragma unroll
        for (int c = 0; c < CLS_MAXC; ++c) {
            const int ch = lane + 64 * c;
            if (ch < nch) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(w + (size_t)ch * 4);
                a += v[c][0] * t[0] + v[c][1] * t[1] + v[c][2] * t[2] + v[c][3] * t[3];
            }
        }
        a = wave_sum(a);
        if (lane == 0) logits[(size_t)row * K + k] = a + (bc ? bc[k] : 0.f);
    }
}

constexpr float kLog2e = 1.4426950408889634f;

// multi_label = 1: one thread per pair, softmax over (contradiction, entailment), the entailment share
__global__ __launch_bounds__(256) void nli_pair_kernel(const float* __restrict__ logits, float* __restrict__ probs, int n, int K, int entail_id, int contra_id) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float en = logits[(size_t)i * K + entail_id], co = logits[(size_t)i * K + contra_id];
    const float m = fmaxf(en, co);
    const float pe = exp2f((en - m) * kLog2e), pc = exp2f((co - m) * kLog2e);
    probs[i] = pe / (pe + pc);
}

// multi_label = 0: one wave per text, softmax of the entailment logits over its Lb labels
__global__ __launch_bounds__(256) void nli_text_kernel(const float* __restrict__ logits, float* __restrict__ probs, int T, int Lb, int K, int entail_id) {
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= T) return;
    const int lane = threadIdx.x & 63;
    const float* l = logits + (size_t)t * Lb * K + entail_id;
    float m = -INFINITY;
    for (int j = lane; j < Lb; j += 64) m = fmaxf(m, l[(size_t)j * K]);
    m = wave_max(m);
    float s = 0.f;
    for (int j = lane; j < Lb; j += 64) s += exp2f((l[(size_t)j * K] - m) * kLog2e);
    s = wave_sum(s);
    for (int j = lane; j < Lb; j += 64) probs[(size_t)t * Lb + j] = exp2f((l[(size_t)j * K] - m) * kLog2e) / s;
}

}  // namespace

const char* glc_launch_cls_head(hipStream_t st, const float* X, const float* norm_w, const float* norm_b, const float* cls_w, const float* cls_b,
                                float* logits, int B, int H, int K, int act, float eps) {
    if (B <= 0 || !X || !cls_w || !logits) return "cls_head: bad args";
    if (H <= 0 || H % 4 || H / 4 > 64 * CLS_MAXC) return "cls_head: hidden size must be a multiple of 4, at most 2048";
    if (K < 1 || K > 1024) return "cls_head: 1 .. 1024 labels";
    if (act < 0 || act > 2) return "cls_head: activation must be 0 (none), 1 (tanh) or 2 (gelu)";
    if (norm_b && !norm_w) return "cls_head: a norm bias without a norm gain";
    hipLaunchKernelGGL(cls_head_kernel, dim3((B + 3) / 4), dim3(256), 0, st, X, norm_w, norm_b, cls_w, cls_b, logits, B, H, K, act, eps);
    return nullptr;
}

const char* glc_launch_nli_scores(hipStream_t st, const float* logits, int T, int Lb, int K, int entail_id, int contra_id, int multi_label, float* probs) {
    if (!logits || !probs || T < 1 || Lb < 1 || K < 2) return "nli_scores: bad args";
    if ((long long)T * Lb > (1ll << 30)) return "nli_scores: too many pairs";
    if (entail_id < 0 || entail_id >= K || contra_id < 0 || contra_id >= K) return "nli_scores: entail_id and contra_id must name one of the K labels";
    if (multi_label) {
        if (entail_id == contra_id) return "nli_scores: entail_id and contra_id must differ";
        hipLaunchKernelGGL(nli_pair_kernel, dim3((T * Lb + 255) / 256), dim3(256), 0, st, logits, probs, T * Lb, K, entail_id, contra_id);
    } else {
        hipLaunchKernelGGL(nli_text_kernel, dim3((T + 3) / 4), dim3(256), 0, st, logits, probs, T, Lb, K, entail_id);
    }
    return nullptr;
}
