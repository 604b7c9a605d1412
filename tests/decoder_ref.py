"""CPU restatement of the decoder backbone (Qwen2 / Llama / Qwen3 arithmetic) + the GLiClass head (torch, fp32 or fp64).

It follows transformers' models/qwen3/modeling_qwen3.py (cited Q3:<line>) and models/llama/modeling_llama.py (LL:<line>) without
importing transformers (the GPU machines may not have it); tests/test_qwen3_host.py pins it on the committed fixtures of
tests/golden/qwen3 and, where transformers is importable, on live HF models.  Right padding, positions 0..S-1 per row:

    x = tok[ids]                                                                    Q3:381
    per layer:  h = RMS(x, input_layernorm)                                         Q3:305   LL:306
                q, k, v = h Wq^T (+ bq), h Wk^T (+ bk), h Wv^T (+ bv)                Q3:252-254 LL:254-256   biases: cfg.attn_bias
                q, k = RMS_head(q, q_norm), RMS_head(k, k_norm)   (cfg.qk_norm)     Q3:237-238, 252-253: over head_dim, per (token, head)
                q, k = RoPE(q), RoPE(k)                                             Q3:140-170 LL:138
                x += softmax(q k^T / sqrt(d) + mask) v Wo^T                         Q3:185-206, 221: grouped queries, causal and key-padding mask
                x += Wd (silu(Wg h2) * Wu h2),  h2 = RMS(x, post_attention_layernorm)    Q3:320, :82   LL:321, :175
    x = RMS(x, norm)                                                                Q3:423   LL:413
RMS(x, w) = w * (x * rsqrt(mean(x^2) + eps)), Q3:50-64 / LL:53-67, eps = cfg.ln_eps everywhere (Qwen3's q_norm / k_norm use rms_norm_eps too).
cfg.causal = 0 drops the causal part of the mask (the bidirectional wrapping, a switch of this project, not of transformers).
The head is tests/modernbert_ref.head, the same restatement for every backbone."""
import numpy as np
import torch

from modernbert_ref import head, _rope_cos_sin, _rot


def _rms(x, w, eps):
    return w * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))


@torch.no_grad()
def backbone(cfg, tensors, ids, mask, dtype=torch.float32, qk_norm=None):
    """-> hidden states [emb, layer 0, ..., layer L-2, RMS_final(layer L-1)] as torch [B, S, H] (glc_debug_get_hidden's numbering).
    qk_norm: override of cfg.qk_norm (tests that show the fixtures see the norm)."""
    class _T:                                                        # tensors converted when a layer asks for them (the full-size models)
        def __getitem__(self, k):
            return torch.from_numpy(np.asarray(tensors[k])).to(dtype)
    t = _T()
    ids_t = torch.from_numpy(np.asarray(ids, np.int64))
    mk = torch.from_numpy(np.asarray(mask, np.int64)) != 0
    B, S = ids_t.shape
    nq, nkv, d, eps = cfg.heads, cfg.kv_heads, cfg.head_dim, cfg.ln_eps
    qkn = cfg.qk_norm if qk_norm is None else qk_norm
    x = torch.from_numpy(np.asarray(tensors["embed_tokens.weight"])[np.asarray(ids, np.int64)]).to(dtype)
    hs = [x]
    cos, sin = _rope_cos_sin(S, d, cfg.rope_theta, dtype)
    allowed = mk[:, None, None, :]                                   # [B, 1, 1, S] keys
    if cfg.causal:
        allowed = allowed & torch.tril(torch.ones(S, S, dtype=torch.bool))[None, None]
    for l in range(cfg.layers):
        p = f"layers.{l}."
        h = _rms(x, t[p + "input_layernorm.weight"], eps)

        def proj(nm, heads):
            y = h @ t[p + f"self_attn.{nm}_proj.weight"].T
            if cfg.attn_bias:
                y = y + t[p + f"self_attn.{nm}_proj.bias"]
            return y.view(B, S, heads, d)
        q, k, v = proj("q", nq), proj("k", nkv), proj("v", nkv)
        if qkn:
            q, k = _rms(q, t[p + "self_attn.q_norm.weight"], eps), _rms(k, t[p + "self_attn.k_norm.weight"], eps)
        q, k, v = q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)      # [B, heads, S, d]
        q, k = _rot(q, cos, sin), _rot(k, cos, sin)
        k, v = k.repeat_interleave(nq // nkv, dim=1), v.repeat_interleave(nq // nkv, dim=1)
        sc = (q @ k.transpose(-1, -2)) * d ** -0.5
        sc = sc.masked_fill(~allowed, torch.finfo(dtype).min)
        ctx = torch.softmax(sc, dim=-1) @ v
        x = x + ctx.transpose(1, 2).reshape(B, S, nq * d) @ t[p + "self_attn.o_proj.weight"].T
        h2 = _rms(x, t[p + "post_attention_layernorm.weight"], eps)
        x = x + (torch.nn.functional.silu(h2 @ t[p + "mlp.gate_proj.weight"].T) * (h2 @ t[p + "mlp.up_proj.weight"].T)) @ t[p + "mlp.down_proj.weight"].T
        hs.append(x)
    hs[-1] = _rms(x, t["norm.weight"], eps)
    return hs


def forward(cfg, tensors, ids, mask, dtype=torch.float64, want_hidden=False, qk_norm=None):
    """-> logits [B, C] numpy (and the hidden states as numpy [L + 1, B, S, H] with want_hidden)."""
    hs = backbone(cfg, tensors, ids, mask, dtype, qk_norm)
    logits = head(cfg, tensors, hs[-1], ids, mask).numpy()
    if want_hidden:
        return logits, np.stack([h.numpy() for h in hs])
    return logits
