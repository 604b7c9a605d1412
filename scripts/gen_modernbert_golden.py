"""Regenerates tests/golden/modernbert/*.npz from HuggingFace ModernBertModel (fp32, CPU) + the GLiClass head of oracle/hf_ref.py.

Run in the build container:  python scripts/gen_modernbert_golden.py
Same record keys as oracle/gen_golden.py; weights are not stored — they are reproduced from (config name, seed) by
gliclass.c_amd.weights.make_weights.  The fixtures live in a subdirectory of their own so that the encoder / decoder suites'
golden/*_b*_s*.npz globs do not pick them up.  hidden_samples[l] is the embedding output (l = 0), the output of layer l - 1,
and for l = L the final norm's output (HF last_hidden_state); compare them at attended positions only.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import transformers  # noqa: E402
from transformers import ModernBertConfig, ModernBertModel  # noqa: E402

from gliclass.c_amd.config import CONFIGS  # noqa: E402
from gliclass.c_amd import weights, synth  # noqa: E402
import hf_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "modernbert")
WEIGHT_SEED = 42

# (case name, config, B, S, C, ragged, labels_per_row)
CASES = [
    ("mb_tiny_b3_s200", "mb-tiny", 3, 200, 4, True, [4, 2, 3]),
    ("mb_tiny_b2_s700", "mb-tiny", 2, 700, 3, False, None),
    ("mb_mini_b2_s333", "mb-mini", 2, 333, 3, False, None),
    ("mb_mini_b2_s1100", "mb-mini", 2, 1100, 4, True, [4, 2]),
]


def hf_config(cfg, legacy=False):
    """ModernBertConfig of a GLiClassConfig; legacy: the older config.json keys (global_attn_every_n_layers, *_rope_theta)."""
    kw = dict(vocab_size=cfg.vocab, hidden_size=cfg.hidden, intermediate_size=cfg.inter, num_hidden_layers=cfg.layers,
              num_attention_heads=cfg.heads, norm_eps=cfg.ln_eps, norm_bias=False, attention_bias=False, mlp_bias=False,
              hidden_activation="gelu", local_attention=2 * cfg.local_window, max_position_embeddings=8192,
              pad_token_id=cfg.pad_id, bos_token_id=cfg.cls_id, cls_token_id=cfg.cls_id, sep_token_id=cfg.sep_id,
              eos_token_id=cfg.sep_id, attention_dropout=0.0, embedding_dropout=0.0, mlp_dropout=0.0)
    if legacy:
        kw.update(global_attn_every_n_layers=cfg.global_every, global_rope_theta=cfg.rope_theta, local_rope_theta=cfg.rope_theta_local)
    else:
        kw.update(layer_types=["full_attention" if cfg.is_global_layer(l) else "sliding_attention" for l in range(cfg.layers)],
                  rope_parameters={"full_attention": {"rope_type": "default", "rope_theta": cfg.rope_theta},
                                   "sliding_attention": {"rope_type": "default", "rope_theta": cfg.rope_theta_local}})
    return ModernBertConfig(**kw)


def build_hf_model(cfg, tensors, legacy=False):
    m = ModernBertModel(hf_config(cfg, legacy)).eval().float()
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
        print(name, "logits", np.round(logits[0], 4), "bytes", os.path.getsize(os.path.join(OUT, name + ".npz")))


if __name__ == "__main__":
    main()
