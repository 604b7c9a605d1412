"""CPU restatement (float64) of the sequence-classification head (head_kind = 1) over the backbone restatements of this directory, and
of the zero-shot NLI reduction.  tests/test_seqcls_host.py pins it on the committed transformers fixtures of tests/golden/seqcls
(scripts/gen_seqcls_golden.py); tests/test_gpu_seqcls.py runs the engine against it.

    pooled = hidden[:, 0] ('first') or the masked mean over the attended tokens ('avg')
    x = pooled W_dense^T + b_dense (cls_dense);  x = tanh(x) | gelu_erf(x) (cls_act);  x = LayerNorm(x) (cls_norm, eps = ln_eps)
    logits = x W_cls^T + b_cls                                  [B, K]

Backbones: tests/bert_ref.py (BERT / RoBERTa / XLM-R), tests/modernbert_ref.py (ModernBERT) and, for DeBERTa-v2/v3, the restatement of
transformers' models/deberta_v2/modeling_deberta_v2.py below (disentangled attention with shared keys, c2p + p2c, log buckets, the
relative embeddings through the encoder's LayerNorm) — there is no other Python restatement of that backbone outside oracle/."""
import numpy as np
import torch

import bert_ref
import modernbert_ref
from gliclass.c_amd.config import BACKBONE_BERT, BACKBONE_DEBERTA, BACKBONE_MODERNBERT, POOL_AVG, POOL_FIRST

_HEAD = ("cls.dense.weight", "cls.dense.bias", "cls.norm.weight", "cls.norm.bias", "cls.classifier.weight", "cls.classifier.bias")


def _ln(x, g, b, eps):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    y = (x - mu) / np.sqrt(var + eps) * g
    return y if b is None else y + b


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(torch.from_numpy(np.ascontiguousarray(x)) / np.sqrt(2.0)).numpy())


def _log_bucket(rel, bucket_size, max_position):
    """make_log_bucket_position (float32 arithmetic, as torch runs it)"""
    rel = rel.astype(np.int64)
    mid = bucket_size // 2
    sign = np.sign(rel)
    abs_pos = np.where((rel < mid) & (rel > -mid), mid - 1, np.abs(rel)).astype(np.float32)
    log_pos = np.ceil(np.log(abs_pos / np.float32(mid)) / np.log(np.float32((max_position - 1) / mid)) * np.float32(mid - 1)) + mid
    return np.where(abs_pos <= mid, rel, (log_pos * sign).astype(np.int64))


def deberta_backbone(cfg, tensors, ids, mask):
    """-> last hidden state [B, S, H] float64 of DebertaV2Model (relative_attention, pos_att_type c2p|p2c, share_att_key,
    norm_rel_ebd layer_norm, position_biased_input false, no conv layer, no token types)"""
    t = {k: np.asarray(v, np.float64) for k, v in tensors.items() if k.startswith(("embeddings.", "encoder."))}
    ids = np.asarray(ids, np.int64)
    mk = np.asarray(mask, np.float64)
    B, S = ids.shape
    H, nh, d, eps = cfg.hidden, cfg.heads, cfg.head_dim, cfg.ln_eps
    span = cfg.att_span
    x = _ln(t["embeddings.word_embeddings.weight"][ids], t["embeddings.LayerNorm.weight"], t["embeddings.LayerNorm.bias"], eps) * mk[..., None]
    rel = _ln(t["encoder.rel_embeddings.weight"][:2 * span], t["encoder.LayerNorm.weight"], t["encoder.LayerNorm.bias"], eps)
    q_idx = np.arange(S)[:, None] - np.arange(S)[None, :]
    if cfg.pos_buckets > 0:
        q_idx = _log_bucket(q_idx, cfg.pos_buckets, cfg.max_rel_pos)
    delta = np.clip(q_idx + span, 0, 2 * span - 1)                       # [q, k]: the row of the relative table for (q - k)
    pair_ok = (mk[:, :, None] * mk[:, None, :])[:, None] > 0            # [B, 1, q, k]: XSoftmax masks padded queries and keys
    scale = np.sqrt(3.0 * d)

    def heads(z):
        return z.reshape(z.shape[:-1] + (nh, d))
    for l in range(cfg.layers):
        p = f"encoder.layer.{l}."
        wq, bq = t[p + "attention.self.query_proj.weight"], t[p + "attention.self.query_proj.bias"]
        wk, bk = t[p + "attention.self.key_proj.weight"], t[p + "attention.self.key_proj.bias"]
        q = heads(x @ wq.T + bq).transpose(0, 2, 1, 3)
        k = heads(x @ wk.T + bk).transpose(0, 2, 1, 3)
        v = heads(x @ t[p + "attention.self.value_proj.weight"].T + t[p + "attention.self.value_proj.bias"]).transpose(0, 2, 1, 3)
        pk = heads(rel @ wk.T + bk).transpose(1, 0, 2)                  # [nh, 2 span, d]: shared key projection of the relative table
        pq = heads(rel @ wq.T + bq).transpose(1, 0, 2)
        sc = q @ k.transpose(0, 1, 3, 2)
        c2p = np.einsum("bhqd,hrd->bhqr", q, pk)                        # query content x relative key at delta(q, k)
        sc = sc + np.take_along_axis(c2p, np.broadcast_to(delta[None, None], (B, nh, S, S)), axis=-1)
        p2c = np.einsum("bhkd,hrd->bhkr", k, pq)                        # key content x relative query at delta(q, k)
        sc = sc + np.take_along_axis(p2c, np.broadcast_to(delta.T[None, None], (B, nh, S, S)), axis=-1).transpose(0, 1, 3, 2)
        sc = np.where(pair_ok, sc / scale, -np.inf)
        m = np.where(np.isfinite(sc.max(-1, keepdims=True)), sc.max(-1, keepdims=True), 0.0)
        pr = np.where(pair_ok, np.exp(sc - m), 0.0)
        pr = pr / np.maximum(pr.sum(-1, keepdims=True), 1e-300)
        ctx = (pr @ v).transpose(0, 2, 1, 3).reshape(B, S, H)
        x = _ln(x + ctx @ t[p + "attention.output.dense.weight"].T + t[p + "attention.output.dense.bias"],
                t[p + "attention.output.LayerNorm.weight"], t[p + "attention.output.LayerNorm.bias"], eps)
        f = _gelu(x @ t[p + "intermediate.dense.weight"].T + t[p + "intermediate.dense.bias"])
        x = _ln(x + f @ t[p + "output.dense.weight"].T + t[p + "output.dense.bias"], t[p + "output.LayerNorm.weight"], t[p + "output.LayerNorm.bias"], eps)
    return x


def last_hidden(cfg, tensors, ids, mask):
    """the backbone's final rows [B, S, H] float64 (what the head pools)"""
    back = {k: v for k, v in tensors.items() if not k.startswith("cls.")}
    if cfg.backbone == BACKBONE_BERT:
        return bert_ref.backbone(cfg, back, ids, mask)[-1]
    if cfg.backbone == BACKBONE_MODERNBERT:
        return modernbert_ref.backbone(cfg, back, np.asarray(ids, np.int64), np.asarray(mask, np.int64), torch.float64)[-1].numpy()
    assert cfg.backbone == BACKBONE_DEBERTA, "no sequence-classification head on this backbone"
    return deberta_backbone(cfg, back, ids, mask)


def head(cfg, tensors, hidden, mask, act=None, norm=None, dense_bias=True):
    """hidden [B, S, H] float64 -> logits [B, K].  act / norm / dense_bias override the config (the fixture generator's and the tests'
    "does the fixture see this stage" checks)."""
    t = {k: (None if tensors.get(k) is None else np.asarray(tensors[k], np.float64)) for k in _HEAD}
    act = cfg.cls_act if act is None else act
    norm = cfg.cls_norm if norm is None else norm
    mk = np.asarray(mask, np.float64)
    if cfg.pooling == POOL_FIRST:
        x = hidden[:, 0]
    else:
        assert cfg.pooling == POOL_AVG
        x = (hidden * mk[..., None]).sum(1) / mk.sum(1, keepdims=True)
    if cfg.cls_dense:
        x = x @ t["cls.dense.weight"].T
        if dense_bias and t["cls.dense.bias"] is not None:
            x = x + t["cls.dense.bias"]
    x = np.tanh(x) if act == 1 else _gelu(x) if act == 2 else x
    if norm:
        x = _ln(x, t["cls.norm.weight"], t["cls.norm.bias"], cfg.ln_eps)
    x = x @ t["cls.classifier.weight"].T
    return x if t["cls.classifier.bias"] is None else x + t["cls.classifier.bias"]


def forward(cfg, tensors, ids, mask, **kw):
    """-> logits [B, K] float64"""
    return head(cfg, tensors, last_hidden(cfg, tensors, ids, mask), mask, **kw)


def probs(logits):
    """what the tests compare: softmax over the K labels, sigmoid for K = 1"""
    z = np.asarray(logits, np.float64)
    if z.shape[-1] == 1:
        return 1.0 / (1.0 + np.exp(-z))
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def nli_scores(logits, T, Lb, entail_id, contra_id, multi_label):
    """transformers/pipelines/zero_shot_classification.py ZeroShotClassificationPipeline.postprocess, in float64: logits [T * Lb, K] are
    reshaped to (T, Lb, K); multi_label (or a single label): entail_contr_logits = reshaped[..., [contradiction_id, entailment_id]],
    scores = exp(.) / exp(.).sum(-1), scores[..., 1]; else entail_logits = reshaped[..., entailment_id], scores = softmax over the labels.
    (The pipeline treats one candidate label as multi_label; the engine's entry takes the flag as given, and so does this function.)"""
    z = np.asarray(logits, np.float64).reshape(T, Lb, -1)
    if multi_label:
        ec = z[..., [contra_id, entail_id]]
        e = np.exp(ec - ec.max(-1, keepdims=True))
        return (e / e.sum(-1, keepdims=True))[..., 1]
    en = z[..., entail_id]
    e = np.exp(en - en.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)
