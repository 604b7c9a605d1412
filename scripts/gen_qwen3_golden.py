"""Regenerates tests/golden/qwen3/*.npz from HuggingFace Qwen3Model / LlamaModel (fp32, CPU) + the GLiClass head of oracle/hf_ref.py.

Run in the build container:  python scripts/gen_qwen3_golden.py
Same record keys as scripts/gen_modernbert_golden.py; weights are not stored — they are reproduced from (config name, seed) by
gliclass.c_amd.weights.make_weights.  The fixtures live in a subdirectory of their own so that the encoder / decoder suites'
golden/*_b*_s*.npz globs do not pick them up.  hidden_samples[l] is the embedding output (l = 0), the output of layer l - 1,
and for l = L the final norm's output (HF last_hidden_state); compare them at attended positions only.

While generating, every Qwen3 case is also run through tests/decoder_ref.py with the QK norm switched off: the fixture must be
missed by more than 100 x the 1e-5 the reference is pinned at, or the fixtures would not see the norm (then pick other gains).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import transformers  # noqa: E402
from transformers import LlamaConfig, LlamaModel, Qwen3Config, Qwen3Model  # noqa: E402

from gliclass.c_amd.config import CONFIGS  # noqa: E402
from gliclass.c_amd import weights, synth  # noqa: E402
import hf_ref  # noqa: E402
import decoder_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "qwen3")
WEIGHT_SEED = 42

# (case name, config, B, S, C, ragged, labels_per_row)
CASES = [
    ("q3_tiny_b2_s7", "q3-tiny", 2, 7, 1, False, [1, 0]),
    ("q3_tiny_b3_s200", "q3-tiny", 3, 200, 4, True, [4, 0, 2]),
    ("q3_mini_b1_s7", "q3-mini", 1, 7, 1, False, None),
    ("q3_mini_b2_s96", "q3-mini", 2, 96, 3, True, [3, 2]),
    ("q3_mini_b3_s200", "q3-mini", 3, 200, 4, True, [4, 1, 3]),
    ("ll_tiny_b2_s7", "ll-tiny", 2, 7, 1, False, [0, 1]),
    ("ll_tiny_b2_s96", "ll-tiny", 2, 96, 2, True, None),
    ("ll_tiny_b3_s200", "ll-tiny", 3, 200, 4, True, [2, 4, 0]),
]


def hf_config(cfg):
    """Qwen3Config (cfg.qk_norm) or LlamaConfig of a decoder GLiClassConfig."""
    kw = dict(vocab_size=cfg.vocab, hidden_size=cfg.hidden, intermediate_size=cfg.inter, num_hidden_layers=cfg.layers,
              num_attention_heads=cfg.heads, num_key_value_heads=cfg.kv_heads, head_dim=cfg.head_dim, hidden_act="silu",
              max_position_embeddings=8192, rms_norm_eps=cfg.ln_eps, attention_bias=bool(cfg.attn_bias), attention_dropout=0.0,
              rope_parameters={"rope_type": "default", "rope_theta": cfg.rope_theta}, tie_word_embeddings=False,
              pad_token_id=cfg.pad_id, bos_token_id=cfg.cls_id, eos_token_id=cfg.sep_id)
    if cfg.qk_norm:
        return Qwen3Config(use_sliding_window=False, **kw)
    return LlamaConfig(mlp_bias=False, **kw)


def build_hf_model(cfg, tensors):
    assert cfg.attn_bias == 0, "attention_bias=True gives o_proj a bias as well, which this project's tensor order does not carry"
    hc = hf_config(cfg)
    m = (Qwen3Model(hc) if cfg.qk_norm else LlamaModel(hc)).eval().float()
    m.config._attn_implementation = "eager"
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in tensors.items() if "projector" not in k and not k.startswith("scorer.")}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and not missing, (missing, unexpected)
    return m


@torch.no_grad()
def hf_forward(cfg, tensors, ids, mask, model):
    """-> logits [B, C], hidden states [L + 1, B, S, H] (emb, layers 0 .. L-2, last_hidden_state)."""
    tid, tm = torch.from_numpy(ids), torch.from_numpy(mask)
    out = model(input_ids=tid, attention_mask=tm, output_hidden_states=True)
    hs = list(out.hidden_states[:cfg.layers]) + [out.last_hidden_state]
    logits = hf_ref.gliclass_head(cfg, tensors, out.last_hidden_state, tid, tm)
    return logits.float().numpy(), np.stack([h.float().numpy() for h in hs])


def sample_positions(S):
    pos = sorted(set([0, 1, 2, 4, 7, 13, S // 3, S // 2, S - 2, S - 1]) & set(range(S)))
    return np.asarray(pos, np.int64)


def main():
    os.makedirs(OUT, exist_ok=True)
    meta = dict(transformers=transformers.__version__, torch=torch.__version__, weight_seed=WEIGHT_SEED)
    models = {}
    for name, cname, B, S, C, ragged, lpr in CASES:
        cfg = CONFIGS[cname]
        if cname not in models:
            w = weights.make_weights(cfg, WEIGHT_SEED)
            models[cname] = (w, build_hf_model(cfg, w))
        w, model = models[cname]
        ids, mask, counts = synth.make_inputs(cfg, B, S, C, seed=1234 + S, ragged=ragged, labels_per_row=lpr)
        logits, hs = hf_forward(cfg, w, ids, mask, model)
        pos = sample_positions(S)
        rec = dict(
            config=np.array(cname), B=B, S=S, ids=ids.astype(np.int32), mask=mask.astype(np.int8),
            counts=counts.astype(np.int32), logits=logits.astype(np.float32),
            probs=(1.0 / (1.0 + np.exp(-logits.astype(np.float64)))).astype(np.float32),
            sample_pos=pos, hidden_samples=hs[:, :, pos, : min(cfg.hidden, 128)].astype(np.float32),
            hidden_abs_sum=np.abs(hs * mask[None, :, :, None]).sum(axis=(2, 3)).astype(np.float64),
            meta=np.array(str(meta)),
        )
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **rec)
        note = ""
        if cfg.qk_norm:
            _, off = decoder_ref.forward(cfg, w, ids, mask, want_hidden=True, qk_norm=0)
            m = mask.astype(bool)[:, pos]
            miss = np.abs(off[:, :, pos, : min(cfg.hidden, 128)] - rec["hidden_samples"])[:, m].max()
            assert miss > 100 * 1e-5, (name, miss)
            note = " miss without the QK norm %.3g" % miss
        print(name, "logits", np.round(logits[0], 4), "bytes", os.path.getsize(os.path.join(OUT, name + ".npz")), note)


if __name__ == "__main__":
    main()
