"""CPU restatement (numpy, float64) of the BERT / RoBERTa / XLM-R backbone + the GLiClass head.

It follows transformers' models/bert/modeling_bert.py (BertModel.forward without the pooler; RoBERTa and XLM-R share the arithmetic
and differ in the position ids, modeling_roberta.py create_position_ids_from_input_ids) without importing transformers;
tests/test_bert_host.py pins it on the committed fixtures of tests/golden/bert (scripts/gen_bert_golden.py):

    x = LN_emb(word[ids] + type[0] + pos[p]);  per layer:  q, k, v = split(x Wqkv^T + bqkv)
    x = LN1(x + softmax(q k^T / sqrt(d) + key mask) v Wo^T + bo);  x = LN2(x + gelu_erf(x W1^T + b1) W2^T + b2)
    p = s (pos_offset 0), or cumsum(ids != pad)[s] (ids[s] != pad) + pad (RoBERTa);  then the head (pooling first / avg / last, scorer 'simple').
Every LayerNorm has gain and bias (eps = cfg.ln_eps).  Token types are always 0."""
import numpy as np
import torch

from gliclass.c_amd.config import POOL_AVG, POOL_FIRST, POOL_LAST, SCORER_DOT


def _ln(x, g, b, eps):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * g + b


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(torch.from_numpy(np.ascontiguousarray(x)) / np.sqrt(2.0)).numpy())


def position_ids(cfg, ids):
    """[B, S] int64: rows of the position table each token reads"""
    ids = np.asarray(ids, np.int64)
    if cfg.pos_offset == 0:
        return np.broadcast_to(np.arange(ids.shape[1], dtype=np.int64), ids.shape).copy()
    tok = (ids != cfg.pad_id).astype(np.int64)
    return np.cumsum(tok, axis=1) * tok + cfg.pad_id


def backbone(cfg, tensors, ids, mask, pos_ids=None):
    """-> list of hidden states [emb, layer 0, ..., layer L-1] as float64 [B, S, H] (HF's hidden_states; the engine's
    glc_debug_get_hidden numbering)."""
    t = {k: np.asarray(v, np.float64) for k, v in tensors.items() if "projector" not in k and not k.startswith("scorer.")}
    ids = np.asarray(ids, np.int64)
    key_ok = np.asarray(mask, np.int64) != 0
    B, S = ids.shape
    H, nh, d, eps = cfg.hidden, cfg.heads, cfg.head_dim, cfg.ln_eps
    p = position_ids(cfg, ids) if pos_ids is None else np.asarray(pos_ids, np.int64)
    assert p.max() < cfg.max_positions
    x = t["embeddings.word_embeddings.weight"][ids] + t["embeddings.token_type_embeddings.weight"][0] + t["embeddings.position_embeddings.weight"][p]
    x = _ln(x, t["embeddings.LayerNorm.weight"], t["embeddings.LayerNorm.bias"], eps)
    hs = [x]
    neg = np.where(key_ok, 0.0, -np.inf)[:, None, None, :]          # additive key mask [B, 1, 1, S]
    for l in range(cfg.layers):
        pre = f"encoder.layer.{l}."
        qkv = (x @ t[pre + "attention.self.Wqkv.weight"].T + t[pre + "attention.self.Wqkv.bias"]).reshape(B, S, 3, nh, d)
        q, k, v = (qkv[:, :, i].transpose(0, 2, 1, 3) for i in range(3))      # [B, nh, S, d]
        sc = q @ k.transpose(0, 1, 3, 2) / np.sqrt(d) + neg
        sc = sc - sc.max(-1, keepdims=True)
        pr = np.exp(sc)
        pr /= pr.sum(-1, keepdims=True)
        ctx = (pr @ v).transpose(0, 2, 1, 3).reshape(B, S, H)
        x = _ln(x + ctx @ t[pre + "attention.output.dense.weight"].T + t[pre + "attention.output.dense.bias"],
                t[pre + "attention.output.LayerNorm.weight"], t[pre + "attention.output.LayerNorm.bias"], eps)
        f = _gelu(x @ t[pre + "intermediate.dense.weight"].T + t[pre + "intermediate.dense.bias"])
        x = _ln(x + f @ t[pre + "output.dense.weight"].T + t[pre + "output.dense.bias"],
                t[pre + "output.LayerNorm.weight"], t[pre + "output.LayerNorm.bias"], eps)
        hs.append(x)
    return hs


def head(cfg, tensors, hidden, ids, mask):
    """hidden [B, S, H] -> logits [B, C] (uni-encoder head, scorer 'simple')"""
    assert cfg.scorer == SCORER_DOT, "bert_ref restates the 'simple' scorer only"
    t = {k: np.asarray(v, np.float64) for k, v in tensors.items() if "projector" in k}
    ids = np.asarray(ids, np.int64)
    mk = np.asarray(mask, np.int64)
    B, S, H = hidden.shape
    cls = ids == cfg.class_token_index
    C = int(cls.sum(-1).max()) if B else 0
    classes = np.zeros((B, C, H))
    for b in range(B):
        pos = np.nonzero(cls[b])[0]
        if not cfg.embed_class_token:
            pos = np.minimum(pos + 1, S - 1)
        classes[b, :len(pos)] = hidden[b, pos]
    if cfg.pooling == POOL_FIRST:
        pooled = hidden[:, 0]
    elif cfg.pooling == POOL_AVG:
        m = mk.astype(np.float64)[..., None]
        pooled = (hidden * m).sum(1) / np.maximum(m.sum(1), 1)
    elif cfg.pooling == POOL_LAST:
        last = np.array([np.nonzero(mk[b])[0][-1] if mk[b].any() else 0 for b in range(B)])
        pooled = hidden[np.arange(B), last]
    else:
        raise NotImplementedError(cfg.pooling)

    def proj(z, pre):
        z = _gelu(z @ t[pre + ".linear_1.weight"].T + t[pre + ".linear_1.bias"])
        return z @ t[pre + ".linear_2.weight"].T + t[pre + ".linear_2.bias"]
    pooled, classes = proj(pooled, "text_projector"), proj(classes, "classes_projector")
    if cfg.normalize_features:
        pooled = pooled / (np.linalg.norm(pooled, axis=-1, keepdims=True) + 1e-8)
        classes = classes / (np.linalg.norm(classes, axis=-1, keepdims=True) + 1e-8)
    logits = np.einsum("bd,bcd->bc", pooled, classes)
    return logits * cfg.logit_scale if cfg.normalize_features else logits


def forward(cfg, tensors, ids, mask, want_hidden=False, pos_ids=None):
    """-> logits [B, C] float64 (and the hidden states [L + 1, B, S, H] with want_hidden)"""
    hs = backbone(cfg, tensors, ids, mask, pos_ids)
    logits = head(cfg, tensors, hs[-1], ids, mask)
    if want_hidden:
        return logits, np.stack(hs)
    return logits


def fixture_model(golden_dir, flavour, head_seed=5):
    """(cfg, tensors) of a committed fixture model ('bert' / 'roberta'): the backbone weights of tests/golden/bert/<flavour>_weights.npz
    (HF-initialised, stored as the float16 values the HF model ran with) and a synthetic head (the fixtures stop at the backbone)."""
    import json
    import os
    from gliclass.c_amd import weights
    z = np.load(os.path.join(golden_dir, "bert", flavour + "_weights.npz"))
    cfg = weights.bert_config_from_hf(json.loads(str(z["config_json"])))
    synth = weights.make_weights(cfg, head_seed)
    t = {n: (z[n].astype(np.float32) if n in z.files else synth[n]) for n, _, _, _ in weights.tensor_specs(cfg)}
    assert all(n in z.files for n in t if "projector" not in n)
    return cfg, t
