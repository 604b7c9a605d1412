#!/usr/bin/env python3
"""Writes tests/golden/t5/*.npz: hidden states of seeded, randomly initialised HF T5EncoderModel instances (the installed
transformers, eager attention) at tiny sizes — the fixtures tests/t5_ref.py is pinned on (tests/test_t5_host.py) and the engine is
run on (tests/test_gpu_t5.py) — and buckets.npz, torch's _relative_position_bucket for every delta in [-4095, 4095] at (32, 128).

  <flavour>_weights.npz   config_json (a GLiClass-style config.json around the backbone's) and every backbone tensor under its blob name
                          (gliclass/c_amd/weights.py; q / k / v and wi_0 / wi_1 fused), as float16: the HF model ran with exactly these values
  <case>.npz              flavour, ids, mask, sample_pos, lhs_samples = last_hidden_state[:, sample_pos] and, for the small cases,
                          hidden_states [L + 1, B, S, H] (embedding, block outputs, the last one behind final_layer_norm)

Every Linear is re-drawn wide enough for peaky attention (T5 does not scale its scores: q and k are drawn narrower than the rest), the
norm gains are moved off 1 and relative_attention_bias is drawn with a spread of a few units.  The script asserts that zeroing the bias
moves every case's last hidden state by more than 0.1.  Usage: python scripts/gen_t5_golden.py [outdir]"""
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
FLAVOURS = {"t5-tiny": dict(model_type="t5", num_heads=2, seed=21), "t5-odd": dict(model_type="mt5", num_heads=3, seed=22)}


def build(flavour):
    from transformers import T5Config, T5EncoderModel
    f = FLAVOURS[flavour]
    torch.manual_seed(f["seed"])
    hc = T5Config(vocab_size=VOCAB, d_model=128, d_kv=64, d_ff=256, num_layers=2, num_heads=f["num_heads"], relative_attention_num_buckets=32,
                  relative_attention_max_distance=128, dropout_rate=0.0, layer_norm_epsilon=1e-6, feed_forward_proj="gated-gelu",
                  is_encoder_decoder=False, use_cache=False, pad_token_id=0, eos_token_id=1)
    model = T5EncoderModel(hc)
    model.config._attn_implementation = "eager"
    with torch.no_grad():
        for name, mod in model.named_modules():
            if isinstance(mod, torch.nn.Linear):
                wide = 0.6 if name.endswith((".q", ".k")) else 1.0
                mod.weight.normal_(0.0, wide / math.sqrt(mod.in_features))
            elif type(mod).__name__ == "T5LayerNorm":
                mod.weight.add_(0.2 * torch.randn_like(mod.weight))
        model.shared.weight.normal_(0.0, 0.6)
        model.encoder.block[0].layer[0].SelfAttention.relative_attention_bias.weight.normal_(0.0, 2.0)
        for p in model.parameters():             # the values a float16 file holds exactly
            p.copy_(p.to(torch.float16).to(torch.float32))
    model.eval()
    enc = dict(model_type=f["model_type"], vocab_size=VOCAB - 2, d_model=128, d_kv=64, d_ff=256, num_layers=2, num_heads=f["num_heads"],
               relative_attention_num_buckets=32, relative_attention_max_distance=128, layer_norm_epsilon=1e-6, feed_forward_proj="gated-gelu",
               dense_act_fn="gelu_new", is_gated_act=True, pad_token_id=0, eos_token_id=1)
    root = dict(encoder_config=enc, architecture_type="uni-encoder", scorer_type="simple", pooling_strategy="first", vocab_size=VOCAB,
                class_token_index=VOCAB - 2, text_token_index=VOCAB - 1, embed_class_token=True, normalize_features=False)
    return model, root


def make_ids(rng, B, S, lens, pad, left=(), holes=()):
    """rows of word ids with <<LABEL>> tokens near the front; lens = attended length per row; left[b] pads in front of row b;
    holes = (row, first, last) interior pad runs"""
    ids = np.full((B, S), pad, np.int64)
    mask = np.zeros((B, S), np.int64)
    for b in range(B):
        l0 = dict(left).get(b, 0)
        n = lens[b]
        row = rng.integers(3, VOCAB - 2, n)
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
def run(model, ids, mask):
    grabbed = []
    hooks = [blk.register_forward_hook(lambda m, i, o: grabbed.append(o[0].numpy().copy())) for blk in model.encoder.block]
    try:
        out = model(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask))
    finally:
        for h in hooks:
            h.remove()
    lhs = out.last_hidden_state.numpy()
    emb = model.shared(torch.from_numpy(ids)).numpy()
    return lhs, np.stack([emb] + grabbed[:-1] + [lhs])


def main(outdir):
    from transformers.models.t5.modeling_t5 import T5Attention
    os.makedirs(outdir, exist_ok=True)
    delta = torch.arange(-4095, 4096)
    np.savez_compressed(os.path.join(outdir, "buckets.npz"), num_buckets=32, max_distance=128, delta=delta.numpy().astype(np.int32),
                        bucket=T5Attention._relative_position_bucket(delta, True, 32, 128).numpy().astype(np.int8))
    rng = np.random.default_rng(20240611)
    cases = {"t5-tiny": [("tiny_s1", make_ids(rng, 1, 1, [1], 0)), ("tiny_s33", make_ids(rng, 2, 33, [33, 20], 0)),
                         ("tiny_s130", make_ids(rng, 2, 130, [130, 97], 0))],
             "t5-odd": [("odd_rpad", make_ids(rng, 3, 40, [40, 25, 9], 0)),
                        ("odd_lpad", make_ids(rng, 3, 40, [40, 33, 30], 0, left=((1, 7),), holes=((2, 10, 15),)))]}
    for flavour in FLAVOURS:
        model, root = build(flavour)
        cfg = weights.t5_config_from_hf(root)
        t = weights.from_state_dict(model.state_dict(), cfg, names=[n for n, _, _, _ in weights.tensor_specs(cfg) if "projector" not in n])
        np.savez(os.path.join(outdir, flavour + "_weights.npz"), config_json=json.dumps(root), **{k: v.astype(np.float16) for k, v in t.items()})
        rb = model.encoder.block[0].layer[0].SelfAttention.relative_attention_bias.weight
        for name, (ids, mask) in cases[flavour]:
            lhs, hs = run(model, ids, mask)
            S = ids.shape[1]
            pos = np.unique(np.concatenate([np.arange(min(S, 8)), np.arange(max(S - 4, 0), S), rng.integers(0, S, 8)]))
            rec = dict(flavour=flavour, ids=ids.astype(np.int32), mask=mask.astype(np.int8), sample_pos=pos.astype(np.int32), lhs_samples=lhs[:, pos])
            if S <= 64:
                rec["hidden_states"] = hs
            np.savez_compressed(os.path.join(outdir, name + ".npz"), **rec)
            if S > 1:           # the fixture sees the bias (one token: softmax over one key, the bias cancels)
                keep = rb.detach().clone()
                with torch.no_grad():
                    rb.zero_()
                lhs0, _ = run(model, ids, mask)
                with torch.no_grad():
                    rb.copy_(keep)
                diff = np.abs(lhs0 - lhs)[mask.astype(bool)].max()
                assert diff > 0.1, (name, diff)
                print(name, "zeroing relative_attention_bias moves the attended rows by", diff)
            print(name, ids.shape, "written")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "t5"))
