"""CPU restatement (numpy, float64) of the T5 v1.1 / mT5 encoder backbone + the GLiClass head.

It follows transformers' models/t5/modeling_t5.py (T5EncoderModel: the encoder T5Stack) without importing transformers;
tests/test_t5_host.py pins it on the committed fixtures of tests/golden/t5 (scripts/gen_t5_golden.py):

    x = shared[ids];  per block:  q, k, v = split(RMS1(x) Wqkv^T)
    x = x + softmax(q k^T + rel_bias[bucket(k - q), head] + key mask) v Wo^T;   x = x + (gelu_new(RMS2(x) Wi0^T) * RMS2(x) Wi1^T) Wd^T
    then final_layer_norm, then the head (pooling first / avg / last, scorer 'simple').
RMS is T5LayerNorm (gain only, eps = cfg.ln_eps); the scores are not scaled; rel_bias is block 0's table, shared by every block;
bucket() is T5Attention._relative_position_bucket with bidirectional=True (float32 log arithmetic, as torch evaluates it)."""
import numpy as np

import bert_ref

head = bert_ref.head


def _rms(x, g, eps):
    return x / np.sqrt((x * x).mean(-1, keepdims=True) + eps) * g


def gelu_new(x):
    return 0.5 * x * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)))


def bucket(delta, num_buckets=32, max_distance=128):
    """_relative_position_bucket(key - query), bidirectional: int64 array in, int64 buckets out.  The log branch is evaluated in
    float32 step by step, as torch does (a float32 tensor divided by float32(math.log(max_distance / max_exact)))."""
    delta = np.asarray(delta, np.int64)
    half = num_buckets // 2
    max_exact = half // 2
    out = np.where(delta > 0, half, 0).astype(np.int64)
    a = np.abs(delta)
    with np.errstate(divide="ignore"):
        lg = np.log(a.astype(np.float32) / np.float32(max_exact)) / np.float32(np.log(max_distance / max_exact)) * np.float32(half - max_exact)
    big = max_exact + np.where(a > 0, lg, 0).astype(np.int64)
    return out + np.where(a < max_exact, a, np.minimum(big, half - 1))


def backbone(cfg, tensors, ids, mask, zero_bias=False):
    """-> list of hidden states [emb, block 0, ..., block L-2, final_layer_norm(block L-1)] as float64 [B, S, H] (the engine's
    glc_debug_get_hidden numbering on the pre-norm backbones)."""
    t = {k: np.asarray(v, np.float64) for k, v in tensors.items() if "projector" not in k and not k.startswith("scorer.")}
    ids = np.asarray(ids, np.int64)
    key_ok = np.asarray(mask, np.int64) != 0
    B, S = ids.shape
    nh, d, eps = cfg.heads, cfg.head_dim, cfg.ln_eps
    x = t["shared.weight"][ids]
    hs = [x]
    pos = np.arange(S)
    rb = t["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"]          # [buckets, heads]
    bias = rb[bucket(pos[None, :] - pos[:, None], cfg.rel_buckets, cfg.rel_max_distance)].transpose(2, 0, 1)      # [nh, q, k]
    if zero_bias:
        bias = bias * 0.0
    neg = np.where(key_ok, 0.0, -np.inf)[:, None, None, :]          # additive key mask [B, 1, 1, S]
    for l in range(cfg.layers):
        pre = f"encoder.block.{l}."
        n = _rms(x, t[pre + "layer.0.layer_norm.weight"], eps)
        qkv = (n @ t[pre + "layer.0.SelfAttention.Wqkv.weight"].T).reshape(B, S, 3, nh, d)
        q, k, v = (qkv[:, :, i].transpose(0, 2, 1, 3) for i in range(3))      # [B, nh, S, d]
        sc = q @ k.transpose(0, 1, 3, 2) + bias[None] + neg
        sc = sc - sc.max(-1, keepdims=True)
        pr = np.exp(sc)
        pr /= pr.sum(-1, keepdims=True)
        ctx = (pr @ v).transpose(0, 2, 1, 3).reshape(B, S, nh * d)
        x = x + ctx @ t[pre + "layer.0.SelfAttention.o.weight"].T
        n = _rms(x, t[pre + "layer.1.layer_norm.weight"], eps)
        gu = n @ t[pre + "layer.1.DenseReluDense.Wgu.weight"].T
        x = x + (gelu_new(gu[..., :cfg.inter]) * gu[..., cfg.inter:]) @ t[pre + "layer.1.DenseReluDense.wo.weight"].T
        hs.append(x)
    hs[-1] = _rms(x, t["encoder.final_layer_norm.weight"], eps) if cfg.layers else hs[-1]
    return hs


def forward(cfg, tensors, ids, mask, want_hidden=False, zero_bias=False):
    """-> logits [B, C] float64 (and the hidden states [L + 1, B, S, H] with want_hidden)"""
    hs = backbone(cfg, tensors, ids, mask, zero_bias)
    logits = head(cfg, tensors, hs[-1], ids, mask)
    if want_hidden:
        return logits, np.stack(hs)
    return logits


def fixture_model(golden_dir, flavour, head_seed=5):
    """(cfg, tensors) of a committed fixture model ('t5-tiny' / 't5-odd'): the backbone weights of tests/golden/t5/<flavour>_weights.npz
    (HF-initialised, stored as the float16 values the HF model ran with) and a synthetic head (the fixtures stop at the backbone)."""
    import json
    import os
    from gliclass.c_amd import weights
    z = np.load(os.path.join(golden_dir, "t5", flavour + "_weights.npz"))
    cfg = weights.t5_config_from_hf(json.loads(str(z["config_json"])))
    synth = weights.make_weights(cfg, head_seed)
    t = {n: (z[n].astype(np.float32) if n in z.files else synth[n]) for n, _, _, _ in weights.tensor_specs(cfg)}
    assert all(n in z.files for n in t if "projector" not in n)
    return cfg, t
