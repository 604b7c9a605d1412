#!/usr/bin/env python3
"""Writes tests/golden/bert/*.npz: hidden states of seeded, randomly initialised HF BertModel / RobertaModel instances (the installed
transformers, eager attention, no pooler) at tiny sizes — the fixtures tests/bert_ref.py is pinned on (tests/test_bert_host.py) and
the engine is run on (tests/test_gpu_bert.py).

  <flavour>_weights.npz   config_json (a GLiClass-style config.json around the backbone's) and every backbone tensor under its blob name
                          (gliclass/c_amd/weights.py; query / key / value fused), as float16: the HF model ran with exactly these values
  <case>.npz              flavour, ids, mask, sample_pos, lhs_samples = last_hidden_state[:, sample_pos] and, for the small cases,
                          hidden_states [L + 1, B, S, H]

Every Linear is re-drawn wide enough for peaky attention, every bias, LayerNorm gain / bias and the token-type rows are moved away from
their 0 / 1 defaults, so that a dropped bias or type row is visible.  Usage: python scripts/gen_bert_golden.py [outdir]"""
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gliclass.c_amd import weights  # noqa: E402

VOCAB = 300                      # 298 word ids + <<LABEL>> (298) + <<SEP>> (299)
DIMS = dict(hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=256, vocab_size=VOCAB,
            hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, hidden_act="gelu")


def build(flavour, seed):
    from transformers import BertConfig, BertModel, RobertaConfig, RobertaModel
    torch.manual_seed(seed)
    if flavour == "bert":
        hc = BertConfig(max_position_embeddings=160, type_vocab_size=2, layer_norm_eps=1e-12, pad_token_id=0, **DIMS)
        model = BertModel(hc, add_pooling_layer=False)
    else:
        hc = RobertaConfig(max_position_embeddings=64, type_vocab_size=1, layer_norm_eps=1e-5, pad_token_id=1, bos_token_id=0, eos_token_id=2, **DIMS)
        model = RobertaModel(hc, add_pooling_layer=False)
    model.config._attn_implementation = "eager"
    with torch.no_grad():
        for name, mod in model.named_modules():
            if isinstance(mod, torch.nn.Linear):
                wide = 1.6 if name.endswith(("query", "key")) else 1.0
                mod.weight.normal_(0.0, wide / math.sqrt(mod.in_features))
                mod.bias.normal_(0.0, 0.1)
            elif isinstance(mod, torch.nn.LayerNorm):
                mod.weight.add_(0.2 * torch.randn_like(mod.weight))
                mod.bias.add_(0.1 * torch.randn_like(mod.bias))
        emb = model.embeddings
        emb.word_embeddings.weight.normal_(0.0, 0.6)
        emb.position_embeddings.weight.normal_(0.0, 0.3)
        emb.token_type_embeddings.weight.normal_(0.1, 0.2)
        for p in model.parameters():             # the values a float16 file holds exactly
            p.copy_(p.to(torch.float16).to(torch.float32))
    model.eval()
    enc = {k: v for k, v in hc.to_dict().items() if k in (
        "model_type", "hidden_size", "num_attention_heads", "num_hidden_layers", "intermediate_size", "hidden_act", "layer_norm_eps",
        "max_position_embeddings", "type_vocab_size", "pad_token_id", "position_embedding_type")}
    enc.update(vocab_size=VOCAB - 2, cls_token_id=0 if flavour != "bert" else 1, sep_token_id=2)
    enc.setdefault("position_embedding_type", "absolute")
    root = dict(encoder_config=enc, architecture_type="uni-encoder", scorer_type="simple", pooling_strategy="first", vocab_size=VOCAB,
                class_token_index=VOCAB - 2, text_token_index=VOCAB - 1, embed_class_token=True, normalize_features=False)
    return model, root


def make_ids(rng, B, S, lens, pad, cls, left=(), holes=()):
    """rows of word ids with <<LABEL>> tokens near the front; lens = attended length per row; left[b] pads in front of row b;
    holes = (row, first, last) interior pad runs"""
    ids = np.full((B, S), pad, np.int64)
    mask = np.zeros((B, S), np.int64)
    for b in range(B):
        l0 = dict(left).get(b, 0)
        n = lens[b]
        row = rng.integers(3, VOCAB - 2, n)
        row[0] = cls
        for p in (1, 4):
            if p < n - 1:
                row[p] = VOCAB - 2
        if n == 1:
            row[0] = VOCAB - 2
        ids[b, l0:l0 + n] = row
        mask[b, l0:l0 + n] = 1
    for b, a, z in holes:
        ids[b, a:z] = pad
        mask[b, a:z] = 0
    return ids, mask


@torch.no_grad()
def run(model, ids, mask, position_ids=None):
    kw = {} if position_ids is None else {"position_ids": torch.from_numpy(position_ids)}
    out = model(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask), output_hidden_states=True, **kw)
    return out.last_hidden_state.numpy(), np.stack([h.numpy() for h in out.hidden_states])


def main(outdir):
    os.makedirs(outdir, exist_ok=True)
    rng = np.random.default_rng(20240607)
    for flavour, seed in (("bert", 11), ("roberta", 12)):
        model, root = build(flavour, seed)
        cfg = weights.bert_config_from_hf(root)
        t = weights.from_state_dict(model.state_dict(), cfg, names=[n for n, _, _, _ in weights.tensor_specs(cfg) if "projector" not in n])
        np.savez(os.path.join(outdir, flavour + "_weights.npz"), config_json=json.dumps(root), **{k: v.astype(np.float16) for k, v in t.items()})
        pad, cls = cfg.pad_id, cfg.cls_id
        if flavour == "bert":
            cases = [("bert_s1", make_ids(rng, 1, 1, [1], pad, cls)), ("bert_s33", make_ids(rng, 2, 33, [33, 20], pad, cls)),
                     ("bert_s130", make_ids(rng, 2, 130, [130, 97], pad, cls))]
        else:
            cases = [("roberta_rpad", make_ids(rng, 3, 40, [40, 25, 9], pad, cls)),
                     ("roberta_lpad", make_ids(rng, 3, 40, [40, 33, 30], pad, cls, left=((1, 7),), holes=((2, 10, 15),)))]
        for name, (ids, mask) in cases:
            lhs, hs = run(model, ids, mask)
            assert np.array_equal(lhs, hs[-1])
            S = ids.shape[1]
            pos = np.unique(np.concatenate([np.arange(min(S, 8)), np.arange(max(S - 4, 0), S), rng.integers(0, S, 8)]))
            rec = dict(flavour=flavour, ids=ids.astype(np.int32), mask=mask.astype(np.int8), sample_pos=pos.astype(np.int32), lhs_samples=lhs[:, pos])
            if S <= 64:
                rec["hidden_states"] = hs
            np.savez_compressed(os.path.join(outdir, name + ".npz"), **rec)
            if name == "roberta_lpad":
                # the fixture sees the positions: with arange + pos_offset in place of the cumulative ids the padded rows move
                naive = np.broadcast_to(np.arange(S, dtype=np.int64) + cfg.pos_offset, ids.shape).copy()
                lhs2, _ = run(model, ids, mask, position_ids=naive)
                diff = np.abs(lhs2 - lhs)[mask.astype(bool)].max()
                assert diff > 1e-2, diff
                print("roberta_lpad: arange positions move the attended rows by", diff)
            print(name, ids.shape, "written")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "bert"))
