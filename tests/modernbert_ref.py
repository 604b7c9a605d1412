"""CPU restatement of the ModernBERT backbone + the GLiClass head (torch, fp32 or fp64), for shapes no fixture covers.

It follows transformers' models/modernbert/modeling_modernbert.py (ModernBertModel.forward) without importing transformers
(the GPU machines may not have it); tests/test_modernbert_host.py pins it on the committed fixtures and, where transformers is
importable, on a live HF model.  Right padding, positions 0..S-1 per row:

    x = LN_emb(tok[ids]);  per layer l:  h = x (l = 0) or LN_attn(x);  q, k, v = split(h Wqkv^T);  RoPE(theta_l) on q, k;
    x += softmax(q k^T / sqrt(d) + key mask [+ |q - k| > W on local layers]) v Wo^T;  x += Wo_mlp (gelu(u) * g), [u | g] = LN_mlp(x) Wi^T
    x = LN_final(x);  then the head (pooling first / avg / last, scorer 'simple').
Every LayerNorm is without bias (eps = cfg.ln_eps)."""
import numpy as np
import torch

from gliclass.c_amd.config import POOL_AVG, POOL_FIRST, POOL_LAST, SCORER_DOT


def _ln(x, w, eps):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), w, None, eps)


def _rope_cos_sin(S, d, theta, dtype):
    inv = 1.0 / (theta ** (torch.arange(0, d, 2, dtype=torch.int64).to(torch.float32) / d))    # float32 as HF computes it
    f = torch.outer(torch.arange(S, dtype=torch.float32), inv)
    emb = torch.cat([f, f], dim=-1)
    return emb.cos().to(dtype), emb.sin().to(dtype)


def _rot(x, cos, sin):
    h = x.shape[-1] // 2
    return x * cos + torch.cat([-x[..., h:], x[..., :h]], dim=-1) * sin


@torch.no_grad()
def backbone(cfg, tensors, ids, mask, dtype=torch.float32):
    """-> list of hidden states [emb, layer 0, ..., layer L-2, LN_final(layer L-1)] as torch [B, S, H] (the engine's
    glc_debug_get_hidden numbering: the last entry is the final norm's output, as HF's last_hidden_state)."""
    t = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in tensors.items()}
    ids_t = torch.from_numpy(np.asarray(ids, np.int64))
    mk = torch.from_numpy(np.asarray(mask, np.int64)) != 0
    B, S = ids_t.shape
    H, nh, d, eps = cfg.hidden, cfg.heads, cfg.head_dim, cfg.ln_eps
    x = _ln(t["embeddings.tok_embeddings.weight"][ids_t], t["embeddings.norm.weight"], eps)
    hs = [x]
    q_pos = torch.arange(S)
    far = (q_pos[:, None] - q_pos[None, :]).abs() > cfg.local_window
    key_ok = mk[:, None, None, :]                                  # [B, 1, 1, S]
    tabs = {}
    for l in range(cfg.layers):
        p = f"layers.{l}."
        glob = cfg.is_global_layer(l)
        theta = cfg.rope_theta if glob else cfg.rope_theta_local
        if theta not in tabs:
            tabs[theta] = _rope_cos_sin(S, d, theta, dtype)
        cos, sin = tabs[theta]
        h = x if l == 0 else _ln(x, t[p + "attn_norm.weight"], eps)
        qkv = (h @ t[p + "attn.Wqkv.weight"].T).view(B, S, 3, nh, d)
        q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))   # [B, nh, S, d]
        q, k = _rot(q, cos, sin), _rot(k, cos, sin)
        sc = (q @ k.transpose(-1, -2)) * d ** -0.5
        allowed = key_ok if glob else key_ok & ~far[None, None]
        sc = sc.masked_fill(~allowed, torch.finfo(dtype).min)
        ctx = torch.softmax(sc, dim=-1) @ v
        x = x + ctx.transpose(1, 2).reshape(B, S, H) @ t[p + "attn.Wo.weight"].T
        u, g = (_ln(x, t[p + "mlp_norm.weight"], eps) @ t[p + "mlp.Wi.weight"].T).chunk(2, dim=-1)
        x = x + (torch.nn.functional.gelu(u) * g) @ t[p + "mlp.Wo.weight"].T
        hs.append(x)
    hs[-1] = _ln(x, t["final_norm.weight"], eps)
    return hs


@torch.no_grad()
def head(cfg, tensors, hidden, ids, mask):
    """hidden [B, S, H] torch -> logits [B, C] (uni-encoder head, scorer 'simple'; the restatement of oracle/hf_ref.gliclass_head)."""
    assert cfg.scorer == SCORER_DOT, "modernbert_ref restates the 'simple' scorer only"
    dtype = hidden.dtype
    t = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in tensors.items() if "projector" in k}
    ids_t = torch.from_numpy(np.asarray(ids, np.int64))
    mk = torch.from_numpy(np.asarray(mask, np.int64))
    B, S, H = hidden.shape
    cls = ids_t == cfg.class_token_index
    C = int(cls.sum(-1).max()) if B else 0
    classes = torch.zeros(B, C, H, dtype=dtype)
    for b in range(B):
        pos = torch.nonzero(cls[b]).flatten()
        if not cfg.embed_class_token:
            pos = pos + 1
        classes[b, :len(pos)] = hidden[b, pos]
    if cfg.pooling == POOL_FIRST:
        pooled = hidden[:, 0]
    elif cfg.pooling == POOL_AVG:
        m = mk.to(dtype).unsqueeze(-1)
        pooled = (hidden * m).sum(1) / m.sum(1).clamp(min=1)
    elif cfg.pooling == POOL_LAST:
        last = torch.stack([torch.nonzero(mk[b]).flatten()[-1] if mk[b].any() else torch.tensor(0) for b in range(B)])
        pooled = hidden[torch.arange(B), last]
    else:
        raise NotImplementedError(cfg.pooling)

    def proj(z, pre):
        z = torch.nn.functional.gelu(z @ t[pre + ".linear_1.weight"].T + t[pre + ".linear_1.bias"])
        return z @ t[pre + ".linear_2.weight"].T + t[pre + ".linear_2.bias"]
    pooled, classes = proj(pooled, "text_projector"), proj(classes, "classes_projector")
    if cfg.normalize_features:
        pooled = pooled / (pooled.norm(dim=-1, keepdim=True) + 1e-8)
        classes = classes / (classes.norm(dim=-1, keepdim=True) + 1e-8)
    logits = torch.einsum("bd,bcd->bc", pooled, classes)
    return logits * cfg.logit_scale if cfg.normalize_features else logits


def forward(cfg, tensors, ids, mask, dtype=torch.float64, want_hidden=False):
    """-> logits [B, C] numpy (and the hidden states as numpy [L + 1, B, S, H] with want_hidden)."""
    hs = backbone(cfg, tensors, ids, mask, dtype)
    logits = head(cfg, tensors, hs[-1], ids, mask).numpy()
    if want_hidden:
        return logits, np.stack([h.numpy() for h in hs])
    return logits
