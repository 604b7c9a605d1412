#!/usr/bin/env python3
"""Writes tests/golden/seqcls/<family>.npz: logits of seeded HF *ForSequenceClassification models (the installed transformers, eager
attention, float32) at tiny sizes — the fixtures tests/seqcls_ref.py is pinned on (tests/test_seqcls_host.py) and the engine is run on
(tests/test_gpu_seqcls.py).  They are the first logits of this repository that are pinned end to end on transformers' own numbers.

  family      model class                                   config (dataclasses.replace of)      head
  deberta     DebertaV2ForSequenceClassification            tiny                                 ContextPooler: dense, GELU; K = 3
  bert        BertForSequenceClassification                 bert-tiny with BERT position ids     BertPooler: dense, tanh; K = 2
  roberta     RobertaForSequenceClassification              bert-tiny (RoBERTa position ids)     classifier.dense, tanh, out_proj; K = 3
  modernbert  ModernBertForSequenceClassification (cls)     mb-tiny                              head.dense (no bias), GELU, head.norm (no bias); K = 3
  modernbert_mean   ... classifier_pooling = "mean"         mb-tiny, pooling avg                 the same, masked mean; K = 1

Each file holds the config fields that differ from the named config (config_json), the weight seed, and per case ids, mask and logits: a
few kilobytes.  The weights are NOT stored: gliclass.c_amd.weights.make_weights(cfg, seed) draws them again (the head tensors with a visible
spread), and the generator asserts that the fixture sees every stage of the head: zeroing dense.bias, swapping the activation for the
identity and dropping the norm each move the logits by far more than any test bar.  Usage: python scripts/gen_seqcls_golden.py [outdir]"""
import dataclasses
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from gliclass.c_amd import weights  # noqa: E402
from gliclass.c_amd.config import CONFIGS, POOL_AVG  # noqa: E402

SEED = 77
# family -> (base config, overrides)
FAMILIES = {
    "deberta": ("tiny", dict(head_kind=1, cls_labels=3, cls_act=2, cls_norm=0, cls_dense=1)),
    "bert": ("bert-tiny", dict(head_kind=1, cls_labels=2, cls_act=1, cls_norm=0, cls_dense=1, pad_id=0, cls_id=1, pos_offset=0, max_positions=160)),
    "roberta": ("bert-tiny", dict(head_kind=1, cls_labels=3, cls_act=1, cls_norm=0, cls_dense=1)),
    "modernbert": ("mb-tiny", dict(head_kind=1, cls_labels=3, cls_act=2, cls_norm=1, cls_dense=1)),
    "modernbert_mean": ("mb-tiny", dict(head_kind=1, cls_labels=1, cls_act=2, cls_norm=1, cls_dense=1, pooling=POOL_AVG)),
}
# ModernBERT's head as the published checkpoints have it: classifier_bias = false (no dense bias), norm_bias = false (no norm bias)
ABSENT = {"modernbert": ("cls.dense.bias", "cls.norm.bias"), "modernbert_mean": ("cls.dense.bias", "cls.norm.bias")}


def family_config(family):
    base, over = FAMILIES[family]
    return dataclasses.replace(CONFIGS[base], **over)


def family_weights(family, cfg=None, seed=SEED):
    """the tensors the fixture models ran with: seeded, under blob names; a tensor the class does not have is absent"""
    w = weights.make_weights(cfg or family_config(family), seed)
    for n in ABSENT.get(family, ()):
        w.pop(n, None)
    return w


def model_type(family):
    return {"deberta": "deberta-v2", "bert": "bert", "roberta": "roberta"}.get(family, "modernbert")


def build_hf(family, cfg, w):
    """the HF model class of the family with the tensors w loaded (float32, eval, eager attention)"""
    import transformers as tf
    K, H = cfg.cls_labels, cfg.hidden
    t = {k: torch.from_numpy(np.ascontiguousarray(v, np.float32)) for k, v in w.items()}
    back = {k: v for k, v in t.items() if not k.startswith("cls.")}
    common = dict(vocab_size=cfg.vocab, hidden_size=H, num_hidden_layers=cfg.layers, num_attention_heads=cfg.heads, intermediate_size=cfg.inter,
                  num_labels=K, pad_token_id=cfg.pad_id)
    if family == "deberta":
        hc = tf.DebertaV2Config(max_position_embeddings=cfg.max_rel_pos, relative_attention=True, position_buckets=cfg.pos_buckets, norm_rel_ebd="layer_norm",
                                share_att_key=True, pos_att_type=["p2c", "c2p"], position_biased_input=False, layer_norm_eps=cfg.ln_eps, type_vocab_size=0,
                                hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, hidden_act="gelu", pooler_hidden_size=H, pooler_hidden_act="gelu",
                                pooler_dropout=0.0, **common)
        m = tf.DebertaV2ForSequenceClassification(hc)
        sd = {"deberta." + k: v for k, v in back.items()}
        sd.update({"pooler.dense.weight": t["cls.dense.weight"], "pooler.dense.bias": t["cls.dense.bias"],
                   "classifier.weight": t["cls.classifier.weight"], "classifier.bias": t["cls.classifier.bias"]})
    elif family in ("bert", "roberta"):
        kw = dict(max_position_embeddings=cfg.max_positions, type_vocab_size=cfg.type_vocab, layer_norm_eps=cfg.ln_eps, hidden_dropout_prob=0.0,
                  attention_probs_dropout_prob=0.0, hidden_act="gelu", classifier_dropout=0.0, **common)
        if family == "bert":
            m, pre = tf.BertForSequenceClassification(tf.BertConfig(**kw)), "bert."
        else:
            m, pre = tf.RobertaForSequenceClassification(tf.RobertaConfig(bos_token_id=cfg.cls_id, eos_token_id=cfg.sep_id, **kw)), "roberta."
        sd = {}
        for k, v in back.items():
            if ".attention.self.Wqkv." in k:
                for part, piece in zip(("query", "key", "value"), torch.chunk(v, 3, dim=0)):
                    sd[pre + k.replace("Wqkv", part)] = piece.clone()
            else:
                sd[pre + k] = v
        if family == "bert":
            sd.update({"bert.pooler.dense.weight": t["cls.dense.weight"], "bert.pooler.dense.bias": t["cls.dense.bias"],
                       "classifier.weight": t["cls.classifier.weight"], "classifier.bias": t["cls.classifier.bias"]})
        else:
            sd.update({"classifier.dense.weight": t["cls.dense.weight"], "classifier.dense.bias": t["cls.dense.bias"],
                       "classifier.out_proj.weight": t["cls.classifier.weight"], "classifier.out_proj.bias": t["cls.classifier.bias"]})
    else:
        hc = tf.ModernBertConfig(norm_eps=cfg.ln_eps, norm_bias=False, attention_bias=False, mlp_bias=False, hidden_activation="gelu",
                                 local_attention=2 * cfg.local_window, max_position_embeddings=8192, bos_token_id=cfg.cls_id, cls_token_id=cfg.cls_id,
                                 sep_token_id=cfg.sep_id, eos_token_id=cfg.sep_id, attention_dropout=0.0, embedding_dropout=0.0, mlp_dropout=0.0,
                                 classifier_dropout=0.0, classifier_bias=False, classifier_activation="gelu",
                                 classifier_pooling="mean" if cfg.pooling == POOL_AVG else "cls",
                                 layer_types=["full_attention" if cfg.is_global_layer(l) else "sliding_attention" for l in range(cfg.layers)],
                                 rope_parameters={"full_attention": {"rope_type": "default", "rope_theta": cfg.rope_theta},
                                                  "sliding_attention": {"rope_type": "default", "rope_theta": cfg.rope_theta_local}}, **common)
        m = tf.ModernBertForSequenceClassification(hc)
        sd = {"model." + k: v for k, v in back.items()}
        sd.update({"head.dense.weight": t["cls.dense.weight"], "head.norm.weight": t["cls.norm.weight"],
                   "classifier.weight": t["cls.classifier.weight"], "classifier.bias": t["cls.classifier.bias"]})
    m = m.eval().float()
    m.config._attn_implementation = "eager"
    missing, unexpected = m.load_state_dict(sd, strict=False)
    missing = [k for k in missing if "position_ids" not in k]
    assert not missing and not unexpected, (missing, unexpected)
    return m


def make_case(cfg, B, S, seed, left=None, holes=()):
    """ragged rows of word ids ([CLS] first, [SEP] last, pad_id behind); left = (row, n): n pad tokens in front of that row;
    holes = (row, first, last): interior pad runs"""
    rng = np.random.default_rng(seed)
    ids = np.full((B, S), cfg.pad_id, np.int64)
    mask = np.zeros((B, S), np.int64)
    for b in range(B):
        n = S if b == 0 else int(rng.integers(max(S // 2, 1), S + 1))
        l0 = left[1] if left and left[0] == b else 0
        n = min(n, S - l0)
        row = rng.integers(3, cfg.vocab - 2, n)
        row[0] = cfg.cls_id
        if n > 1:
            row[-1] = cfg.sep_id
        ids[b, l0:l0 + n] = row
        mask[b, l0:l0 + n] = 1
    for b, a, z in holes:
        ids[b, a:z] = cfg.pad_id
        mask[b, a:z] = 0
    return ids, mask


def cases(family, cfg):
    out = [("b1_s1", make_case(cfg, 1, 1, 1)), ("b3_s33", make_case(cfg, 3, 33, 2))]
    if family == "roberta":            # pad runs inside a row: the cumulative position ids of everything behind them move
        out.append(("b3_s40_holes", make_case(cfg, 3, 40, 3, holes=((0, 10, 15), (2, 5, 8)))))
    elif family == "modernbert_mean":  # a left-padded row under the masked mean
        out.append(("b3_s70_lpad", make_case(cfg, 3, 70, 4, left=(1, 9))))
    else:
        out.append(("b2_s130", make_case(cfg, 2, 130, 5)))
    return out


@torch.no_grad()
def hf_logits(model, ids, mask):
    return model(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask)).logits.numpy()


def main(outdir):
    import seqcls_ref
    os.makedirs(outdir, exist_ok=True)
    for family in FAMILIES:
        cfg = family_config(family)
        w = family_weights(family, cfg)
        model = build_hf(family, cfg, w)
        rec = dict(config_json=json.dumps(dict(base=FAMILIES[family][0], overrides=FAMILIES[family][1])), seed=np.int64(SEED),
                   absent=np.array(ABSENT.get(family, ()), dtype="U32"), case_names=np.array([n for n, _ in cases(family, cfg)], dtype="U32"))
        for name, (ids, mask) in cases(family, cfg):
            logits = hf_logits(model, ids, mask)
            rec[name + ".ids"], rec[name + ".mask"], rec[name + ".logits"] = ids.astype(np.int32), mask.astype(np.int8), logits
            ref = seqcls_ref.forward(cfg, w, ids, mask)
            print(f"{family} {name}: logits {logits.shape}, |ref - hf| = {np.abs(ref - logits).max():.2e}")
            # the fixture sees each stage of the head
            w0 = dict(w)
            if "cls.dense.bias" in w0:
                moved = np.abs(seqcls_ref.forward(cfg, w, ids, mask, dense_bias=False) - ref).max()
                assert moved > 1e-2, ("dense.bias", family, name, moved)
            moved = np.abs(seqcls_ref.forward(cfg, w, ids, mask, act=0) - ref).max()
            assert moved > 1e-2, ("activation", family, name, moved)
            if cfg.cls_norm:
                moved = np.abs(seqcls_ref.forward(cfg, w, ids, mask, norm=0) - ref).max()
                assert moved > 1e-2, ("norm", family, name, moved)
        np.savez_compressed(os.path.join(outdir, family + ".npz"), **rec)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "seqcls"))
