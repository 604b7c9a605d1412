"""Weight blob (.glcw) writer/reader + deterministic synthetic weights.

The reference loads `onnx/model.onnx` (`/root/reference/include/paths.h:5`,
`/root/reference/src/model.c:269`); this engine loads a flat blob instead:

    [glcw_header 256 B][glcw_tensor x n (160 B each)][pad to 64][tensor data, each 64-B aligned]

Tensor names follow HF `DebertaV2Model.state_dict()` (prefix-free) plus the GLiClass head
(`text_projector.linear_{1,2}`, `classes_projector.linear_{1,2}`), so a converter from a real
`model.safetensors` is a rename (see `from_state_dict`).  The C reader is
`gliclass/c_amd/host/glc_weights.c`; layouts are mirrored in `include/gliclass_hip.h`.
"""
import math
import struct
from typing import Dict, List, Tuple

import numpy as np

from .config import (GLiClassConfig, BACKBONE_DEBERTA, BACKBONE_DECODER, BACKBONE_MODERNBERT, BACKBONE_BERT, BACKBONE_T5, SCORER_WEIGHTED_DOT, SCORER_MLP,
                     SCORER_MLP_HIDDEN, HEAD_SEQCLS, CLS_ACT_TANH, CLS_ACT_GELU, CLS_MAX_LABELS, POOL_FIRST, POOL_AVG)
from . import prng

MAGIC = b"GLCW\x00\x01\x00\x00"
HEADER_BYTES = 256
TENSOR_REC_BYTES = 160
# int32 slots of the header, in order (mirrors struct glcw_header in include/gliclass_hip.h)
_INT_FIELDS = ["vocab", "hidden", "layers", "heads", "head_dim", "inter", "pos_buckets", "max_rel_pos",
               "pad_id", "cls_id", "sep_id", "class_token_index", "text_token_index",
               "pooling", "scorer", "embed_class_token", "normalize_features", "backbone", "kv_heads", "causal"]
_F32_FIELDS = ["ln_eps", "logit_scale", "rope_theta"]
# version 3 (ModernBERT backbone only): + local_window, global_every (int32), rope_theta_local (f32) after the v2 slots
_V3_INT_FIELDS = ["local_window", "global_every"]
_V3_F32_FIELDS = ["rope_theta_local"]
# version 4 (decoder backbones other than Qwen2, i.e. (qk_norm, attn_bias) != (0, 1)): + qk_norm, attn_bias (int32) after the v3 slots
_V4_INT_FIELDS = ["qk_norm", "attn_bias"]
# version 5 (BERT backbone only): + max_positions, type_vocab, pos_offset (int32) after the v4 slots
_V5_INT_FIELDS = ["max_positions", "type_vocab", "pos_offset"]
# version 6 (T5 backbone only): + rel_buckets, rel_max_distance (int32) after the v5 slots
_V6_INT_FIELDS = ["rel_buckets", "rel_max_distance"]
# version 7 (head_kind = 1, the sequence-classification head, only): + head_kind, cls_labels, cls_act, cls_norm, cls_dense (int32) after the v6 slots;
# v7 carries every older slot whatever the backbone
_V7_INT_FIELDS = ["head_kind", "cls_labels", "cls_act", "cls_norm", "cls_dense"]
# the sequence-classification head's tensors in the order of include/gliclass_hip.h (blob names: "cls." + the name there); the biases that a
# checkpoint may switch off (ModernBERT classifier_bias = false: dense.bias; norm_bias = false: norm.bias) are simply absent from the tensor dict and the blob
CLS_HEAD_NAMES = ("cls.dense.weight", "cls.dense.bias", "cls.norm.weight", "cls.norm.bias", "cls.classifier.weight", "cls.classifier.bias")
CLS_OPTIONAL_BIASES = ("cls.dense.bias", "cls.norm.bias", "cls.classifier.bias")


def tensor_specs(cfg: GLiClassConfig) -> List[Tuple[str, Tuple[int, ...], float, float]]:
    """(name, shape, uniform amplitude, mean) for every tensor, in blob order.

    Amplitudes are chosen so random models are numerically *interesting*: attention is peaky
    (q/k targets 2.0 std => score std ~ 2-4 after the 1/sqrt(3d) scale), residual branches are
    O(1), and logits land in the sigmoid's sensitive range (|logit| ~ 1-3).
    """
    H, I, L = cfg.hidden, cfg.inter, cfg.layers
    s3 = math.sqrt(3.0)

    def lin(t, fan_in):
        return s3 * t / math.sqrt(fan_in)

    def head_specs():
        if cfg.head_kind == HEAD_SEQCLS:
            # drawn with a visible spread: a dropped bias, a skipped activation (the dense output has a spread of ~1: tanh and GELU bend it) or a
            # skipped norm (gain around 1.5, bias off zero) moves the logits by tenths
            K = cfg.cls_labels
            out = []
            if cfg.cls_dense:
                out += [("cls.dense.weight", (H, H), lin(1.0, H), 0.0), ("cls.dense.bias", (H,), 0.5, 0.0)]
            if cfg.cls_norm:
                out += [("cls.norm.weight", (H,), 0.5, 1.5), ("cls.norm.bias", (H,), 0.3, 0.1)]
            return out + [("cls.classifier.weight", (K, H), lin(2.0, H), 0.0), ("cls.classifier.bias", (K,), 0.5, 0.0)]
        t2 = math.sqrt(1.5 / math.sqrt(H)) / 0.7
        out = []
        for proj in ("text_projector", "classes_projector"):
            out += [
                (proj + ".linear_1.weight", (H, H), lin(1.0, H), 0.0),
                (proj + ".linear_1.bias", (H,), 0.1, 0.0),
                (proj + ".linear_2.weight", (H, H), lin(t2, H), 0.0),
                (proj + ".linear_2.bias", (H,), 0.02, 0.0),
            ]
        # the scorer's own tensors (include/gliclass_hip.h; mirrors head_spec in host/glc_weights.c)
        if cfg.scorer == SCORER_WEIGHTED_DOT:
            out += [
                ("scorer.proj_text.weight", (2 * H, H), lin(1.0, H), 0.0), ("scorer.proj_text.bias", (2 * H,), 0.05, 0.0),
                ("scorer.proj_label.weight", (2 * H, H), lin(1.0, H), 0.0), ("scorer.proj_label.bias", (2 * H,), 0.05, 0.0),
                ("scorer.out_mlp.0.weight", (4 * H, 3 * H), lin(1.0, 3 * H), 0.0), ("scorer.out_mlp.0.bias", (4 * H,), 0.05, 0.0),
                ("scorer.out_mlp.3.weight", (1, 4 * H), lin(2.0, 4 * H), 0.0), ("scorer.out_mlp.3.bias", (1,), 0.1, 0.0),
            ]
        elif cfg.scorer == SCORER_MLP:
            Mh = SCORER_MLP_HIDDEN
            out += [
                ("scorer.mlp.0.weight", (Mh, 2 * H), lin(1.0, 2 * H), 0.0), ("scorer.mlp.0.bias", (Mh,), 0.05, 0.0),
                ("scorer.mlp.2.weight", (Mh // 2, Mh), lin(1.5, Mh), 0.0), ("scorer.mlp.2.bias", (Mh // 2,), 0.05, 0.0),
                ("scorer.mlp.4.weight", (1, Mh // 2), lin(3.0, Mh // 2), 0.0), ("scorer.mlp.4.bias", (1,), 0.1, 0.0),
            ]
        return out

    if cfg.backbone == BACKBONE_MODERNBERT:
        # HF ModernBertModel.state_dict() names (prefix-free; no biases).  Wqkv rows: Q | K | V; Wi rows: input | gate.
        specs = [("embeddings.tok_embeddings.weight", (cfg.vocab, H), 1.0, 0.0), ("embeddings.norm.weight", (H,), 0.2, 1.0)]
        for i in range(L):
            p = f"layers.{i}."
            if i > 0:
                specs += [(p + "attn_norm.weight", (H,), 0.2, 1.0)]
            specs += [
                (p + "attn.Wqkv.weight", (3 * H, H), lin(1.6, H), 0.0),
                (p + "attn.Wo.weight", (H, H), lin(0.7, H), 0.0),
                (p + "mlp_norm.weight", (H,), 0.2, 1.0),
                (p + "mlp.Wi.weight", (2 * I, H), lin(1.0, H), 0.0),
                (p + "mlp.Wo.weight", (H, I), lin(0.7, I), 0.0),
            ]
        specs += [("final_norm.weight", (H,), 0.2, 1.0)]
        return specs + head_specs()

    if cfg.backbone == BACKBONE_BERT:
        # HF BertModel / RobertaModel / XLMRobertaModel.state_dict() names (prefix-free), with query / key / value fused into Wqkv (rows
        # Q | K | V: from_state_dict and the C importer concatenate them).  The position and token-type rows are drawn smaller than the word
        # rows and with a non-zero mean for the type rows, so that a dropped or mis-indexed row is visible in the output.
        specs = [
            ("embeddings.word_embeddings.weight", (cfg.vocab, H), 1.0, 0.0),
            ("embeddings.position_embeddings.weight", (cfg.max_positions, H), 0.5, 0.0),
            ("embeddings.token_type_embeddings.weight", (cfg.type_vocab, H), 0.3, 0.1),
            ("embeddings.LayerNorm.weight", (H,), 0.2, 1.0),
            ("embeddings.LayerNorm.bias", (H,), 0.1, 0.0),
        ]
        for i in range(L):
            p = f"encoder.layer.{i}."
            specs += [
                (p + "attention.self.Wqkv.weight", (3 * H, H), lin(1.6, H), 0.0),
                (p + "attention.self.Wqkv.bias", (3 * H,), 0.1, 0.0),
                (p + "attention.output.dense.weight", (H, H), lin(1.0, H), 0.0),
                (p + "attention.output.dense.bias", (H,), 0.1, 0.0),
                (p + "attention.output.LayerNorm.weight", (H,), 0.2, 1.0),
                (p + "attention.output.LayerNorm.bias", (H,), 0.1, 0.0),
                (p + "intermediate.dense.weight", (I, H), lin(1.0, H), 0.0),
                (p + "intermediate.dense.bias", (I,), 0.1, 0.0),
                (p + "output.dense.weight", (H, I), lin(1.0, I), 0.0),
                (p + "output.dense.bias", (H,), 0.1, 0.0),
                (p + "output.LayerNorm.weight", (H,), 0.2, 1.0),
                (p + "output.LayerNorm.bias", (H,), 0.1, 0.0),
            ]
        return specs + head_specs()

    if cfg.backbone == BACKBONE_T5:
        # HF T5EncoderModel.state_dict() names, with q / k / v fused into Wqkv (rows q | k | v) and wi_0 / wi_1 into Wgu (rows wi_0 | wi_1):
        # from_state_dict and the C importer concatenate them.  T5 does not scale its scores, so q and k are drawn narrow enough for a
        # score spread of 2-3 (0.6^2 * sqrt(64)); the bias table spreads over a few units, so that a skipped bias is visible.
        inner = cfg.heads * cfg.head_dim
        specs = [("shared.weight", (cfg.vocab, H), 1.0, 0.0),
                 ("encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight", (cfg.rel_buckets, cfg.heads), 3.0, 0.0)]
        for i in range(L):
            p = f"encoder.block.{i}."
            specs += [
                (p + "layer.0.layer_norm.weight", (H,), 0.2, 1.0),
                (p + "layer.0.SelfAttention.Wqkv.weight", (3 * inner, H), lin(0.6, H), 0.0),
                (p + "layer.0.SelfAttention.o.weight", (H, inner), lin(1.0, inner), 0.0),
                (p + "layer.1.layer_norm.weight", (H,), 0.2, 1.0),
                (p + "layer.1.DenseReluDense.Wgu.weight", (2 * I, H), lin(1.0, H), 0.0),
                (p + "layer.1.DenseReluDense.wo.weight", (H, I), lin(0.7, I), 0.0),
            ]
        specs += [("encoder.final_layer_norm.weight", (H,), 0.2, 1.0)]
        return specs + head_specs()

    if cfg.backbone == BACKBONE_DECODER:
        # HF Qwen2Model / LlamaModel / Qwen3Model.state_dict() names (prefix-free).  q/k amplitudes give score std ~ 2-3 after 1/sqrt(d).
        # Qwen3's q_norm / k_norm gains: drawn around 1 like the other norm gains, with a wider spread and another centre for q (1.1 +- 0.4)
        # than for k (0.9 +- 0.3), so that a skipped, swapped or mis-indexed gain is visible in the output.
        nqd, nkvd = cfg.heads * cfg.head_dim, cfg.kv_heads * cfg.head_dim
        specs = [("embed_tokens.weight", (cfg.vocab, H), 1.0, 0.0)]
        for i in range(L):
            p = f"layers.{i}."
            specs += [(p + "input_layernorm.weight", (H,), 0.2, 1.0)]
            for nm, rows, t in (("q", nqd, 1.6), ("k", nkvd, 1.6), ("v", nkvd, 1.0)):
                specs += [(p + f"self_attn.{nm}_proj.weight", (rows, H), lin(t, H), 0.0)]
                if cfg.attn_bias:
                    specs += [(p + f"self_attn.{nm}_proj.bias", (rows,), 0.1, 0.0)]
            if cfg.qk_norm:
                specs += [(p + "self_attn.q_norm.weight", (cfg.head_dim,), 0.4, 1.1), (p + "self_attn.k_norm.weight", (cfg.head_dim,), 0.3, 0.9)]
            specs += [
                (p + "self_attn.o_proj.weight", (H, nqd), lin(0.7, nqd), 0.0),
                (p + "post_attention_layernorm.weight", (H,), 0.2, 1.0),
                (p + "mlp.gate_proj.weight", (I, H), lin(1.0, H), 0.0),
                (p + "mlp.up_proj.weight", (I, H), lin(1.0, H), 0.0),
                (p + "mlp.down_proj.weight", (H, I), lin(0.7, I), 0.0),
            ]
        specs += [("norm.weight", (H,), 0.2, 1.0)]
        return specs + head_specs()

    specs = [
        ("embeddings.word_embeddings.weight", (cfg.vocab, H), 1.0, 0.0),
        ("embeddings.LayerNorm.weight", (H,), 0.2, 1.0),
        ("embeddings.LayerNorm.bias", (H,), 0.1, 0.0),
        ("encoder.rel_embeddings.weight", (2 * cfg.att_span, H), 1.0, 0.0),
        ("encoder.LayerNorm.weight", (H,), 0.2, 1.0),
        ("encoder.LayerNorm.bias", (H,), 0.1, 0.0),
    ]
    for i in range(L):
        p = f"encoder.layer.{i}."
        specs += [
            (p + "attention.self.query_proj.weight", (H, H), lin(2.0, H), 0.0),
            (p + "attention.self.query_proj.bias", (H,), 0.1, 0.0),
            (p + "attention.self.key_proj.weight", (H, H), lin(2.0, H), 0.0),
            (p + "attention.self.key_proj.bias", (H,), 0.1, 0.0),
            (p + "attention.self.value_proj.weight", (H, H), lin(1.0, H), 0.0),
            (p + "attention.self.value_proj.bias", (H,), 0.1, 0.0),
            (p + "attention.output.dense.weight", (H, H), lin(1.0, H), 0.0),
            (p + "attention.output.dense.bias", (H,), 0.1, 0.0),
            (p + "attention.output.LayerNorm.weight", (H,), 0.2, 1.0),
            (p + "attention.output.LayerNorm.bias", (H,), 0.1, 0.0),
            (p + "intermediate.dense.weight", (I, H), lin(1.0, H), 0.0),
            (p + "intermediate.dense.bias", (I,), 0.1, 0.0),
            (p + "output.dense.weight", (H, I), lin(1.0, I), 0.0),
            (p + "output.dense.bias", (H,), 0.1, 0.0),
            (p + "output.LayerNorm.weight", (H,), 0.2, 1.0),
            (p + "output.LayerNorm.bias", (H,), 0.1, 0.0),
        ]
    return specs + head_specs()


def make_weights(cfg: GLiClassConfig, seed: int = 42) -> Dict[str, np.ndarray]:
    out = {}
    for name, shape, amp, mean in tensor_specs(cfg):
        n = int(np.prod(shape))
        out[name] = prng.uniform_f32(seed, name, n, amp, mean).reshape(shape)
    return out


def _pack_header(cfg: GLiClassConfig, n_tensors: int) -> bytes:
    d = cfg.asdict()
    v7 = cfg.head_kind == HEAD_SEQCLS                 # v7 carries every older slot
    v6 = v7 or cfg.backbone == BACKBONE_T5            # v6 carries the v3, v4 and v5 slots too
    v5 = v6 or cfg.backbone == BACKBONE_BERT          # v5 carries the v3 and v4 slots too
    v4 = v5 or (cfg.qk_norm, cfg.attn_bias) != (0, 1)       # Llama / Qwen3 decoders; v4 carries the v3 slots too
    v3 = cfg.backbone == BACKBONE_MODERNBERT          # every other backbone keeps writing byte-identical v2 headers
    b = MAGIC + struct.pack("<II", 7 if v7 else 6 if v6 else 5 if v5 else 4 if v4 else 3 if v3 else 2, n_tensors)     # version 2: + backbone, kv_heads, causal, rope_theta
    b += struct.pack("<%di" % len(_INT_FIELDS), *[int(d[k]) for k in _INT_FIELDS])
    b += struct.pack("<%df" % len(_F32_FIELDS), *[float(d[k]) for k in _F32_FIELDS])
    if v3 or v4:
        b += struct.pack("<%di" % len(_V3_INT_FIELDS), *[int(d[k]) for k in _V3_INT_FIELDS])
        b += struct.pack("<%df" % len(_V3_F32_FIELDS), *[float(d[k]) for k in _V3_F32_FIELDS])
    if v4:
        b += struct.pack("<%di" % len(_V4_INT_FIELDS), *[int(d[k]) for k in _V4_INT_FIELDS])
    if v5:
        b += struct.pack("<%di" % len(_V5_INT_FIELDS), *[int(d[k]) for k in _V5_INT_FIELDS])
    if v6:
        b += struct.pack("<%di" % len(_V6_INT_FIELDS), *[int(d[k]) for k in _V6_INT_FIELDS])
    if v7:
        b += struct.pack("<%di" % len(_V7_INT_FIELDS), *[int(d[k]) for k in _V7_INT_FIELDS])
    assert len(b) <= HEADER_BYTES
    return b + b"\x00" * (HEADER_BYTES - len(b))


def write_blob(path: str, cfg: GLiClassConfig, tensors: Dict[str, np.ndarray]) -> None:
    names = [s[0] for s in tensor_specs(cfg) if not (s[0] in CLS_OPTIONAL_BIASES and tensors.get(s[0]) is None)]
    missing = [n for n in names if n not in tensors]
    if missing:
        raise KeyError(f"missing tensors: {missing[:4]}...")
    table_end = HEADER_BYTES + TENSOR_REC_BYTES * len(names)
    off = (table_end + 63) // 64 * 64
    recs, offs = [], []
    for n in names:
        a = np.ascontiguousarray(tensors[n], dtype=np.float32)
        shape = list(a.shape) + [0] * (4 - a.ndim)
        nm = n.encode("utf-8")
        assert len(nm) < 96
        recs.append(nm + b"\x00" * (96 - len(nm)) + struct.pack("<II4QQQ", 0, a.ndim, *shape, off, a.nbytes) + b"\x00" * 8)
        assert len(recs[-1]) == TENSOR_REC_BYTES
        offs.append(off)
        off = (off + a.nbytes + 63) // 64 * 64
    with open(path, "wb") as f:
        f.write(_pack_header(cfg, len(names)))
        for r in recs:
            f.write(r)
        for n, o in zip(names, offs):
            f.seek(o)
            f.write(np.ascontiguousarray(tensors[n], dtype=np.float32).tobytes())
        f.truncate(off)


def read_blob(path: str) -> Tuple[GLiClassConfig, Dict[str, np.ndarray]]:
    raw = np.fromfile(path, dtype=np.uint8)
    hdr = raw[:HEADER_BYTES].tobytes()
    if hdr[:8] != MAGIC:
        raise ValueError("not a GLCW blob")
    ver, n_t = struct.unpack_from("<II", hdr, 8)
    if ver not in (2, 3, 4, 5, 6, 7):
        raise ValueError(f"unsupported GLCW version {ver}")
    ints = struct.unpack_from("<%di" % len(_INT_FIELDS), hdr, 16)
    flts = struct.unpack_from("<%df" % len(_F32_FIELDS), hdr, 16 + 4 * len(_INT_FIELDS))
    kw = dict(zip(_INT_FIELDS, ints))
    kw.update(dict(zip(_F32_FIELDS, flts)))
    if ver >= 3:
        o3 = 16 + 4 * (len(_INT_FIELDS) + len(_F32_FIELDS))
        kw.update(dict(zip(_V3_INT_FIELDS, struct.unpack_from("<%di" % len(_V3_INT_FIELDS), hdr, o3))))
        kw.update(dict(zip(_V3_F32_FIELDS, struct.unpack_from("<%df" % len(_V3_F32_FIELDS), hdr, o3 + 4 * len(_V3_INT_FIELDS)))))
    if ver >= 4:          # older blobs mean (qk_norm, attn_bias) = (0, 1), the dataclass defaults
        o4 = 16 + 4 * (len(_INT_FIELDS) + len(_F32_FIELDS) + len(_V3_INT_FIELDS) + len(_V3_F32_FIELDS))
        kw.update(dict(zip(_V4_INT_FIELDS, struct.unpack_from("<%di" % len(_V4_INT_FIELDS), hdr, o4))))
    if ver >= 5:
        o5 = 16 + 4 * (len(_INT_FIELDS) + len(_F32_FIELDS) + len(_V3_INT_FIELDS) + len(_V3_F32_FIELDS) + len(_V4_INT_FIELDS))
        kw.update(dict(zip(_V5_INT_FIELDS, struct.unpack_from("<%di" % len(_V5_INT_FIELDS), hdr, o5))))
    if ver >= 6:
        o6 = 16 + 4 * (len(_INT_FIELDS) + len(_F32_FIELDS) + len(_V3_INT_FIELDS) + len(_V3_F32_FIELDS) + len(_V4_INT_FIELDS) + len(_V5_INT_FIELDS))
        kw.update(dict(zip(_V6_INT_FIELDS, struct.unpack_from("<%di" % len(_V6_INT_FIELDS), hdr, o6))))
    if ver >= 7:
        o7 = 16 + 4 * (len(_INT_FIELDS) + len(_F32_FIELDS) + len(_V3_INT_FIELDS) + len(_V3_F32_FIELDS) + len(_V4_INT_FIELDS) + len(_V5_INT_FIELDS) + len(_V6_INT_FIELDS))
        kw.update(dict(zip(_V7_INT_FIELDS, struct.unpack_from("<%di" % len(_V7_INT_FIELDS), hdr, o7))))
    cfg = GLiClassConfig(name="blob", **kw)
    tensors = {}
    for i in range(n_t):
        rec = raw[HEADER_BYTES + i * TENSOR_REC_BYTES: HEADER_BYTES + (i + 1) * TENSOR_REC_BYTES].tobytes()
        name = rec[:96].split(b"\x00", 1)[0].decode()
        _, ndim, s0, s1, s2, s3, off, nb = struct.unpack_from("<II4QQQ", rec, 96)
        shape = (s0, s1, s2, s3)[:ndim]
        tensors[name] = raw[off:off + nb].view(np.float32).reshape(shape)
    return cfg, tensors


def from_state_dict(sd: Dict[str, "np.ndarray"], cfg: GLiClassConfig, names=None) -> Dict[str, np.ndarray]:
    """Rename a (GLiClass or bare backbone) state_dict to blob names.

    Accepts the prefixes HF / gliclass checkpoints use (`deberta.`, `encoder_model.model.`, none).  `names`: the blob names to
    convert (default: every tensor of the config; a bare backbone has no head tensors).
    """
    out = {}
    want = [s[0] for s in tensor_specs(cfg)] if names is None else list(names)
    prefixes = ("", "deberta.", "encoder_model.model.", "model.encoder_model.model.", "model.", "decoder_model.model.") + \
        (_BERT_PREFIXES if cfg.backbone in (BACKBONE_BERT, BACKBONE_T5) else ())

    def find(n):
        for pre in prefixes:
            if pre + n in sd:
                v = sd[pre + n]
                return v.detach().cpu().float().numpy() if hasattr(v, "detach") else np.asarray(v, np.float32)
        raise KeyError(n)

    for n in want:
        if cfg.backbone == BACKBONE_BERT and ".attention.self.Wqkv." in n:      # HF keeps query / key / value apart: rows Q | K | V
            out[n] = np.concatenate([find(n.replace("Wqkv", part)) for part in ("query", "key", "value")], axis=0)
        elif cfg.backbone == BACKBONE_T5 and ".SelfAttention.Wqkv." in n:       # T5Attention q / k / v: rows q | k | v
            out[n] = np.concatenate([find(n.replace("Wqkv", part)) for part in ("q", "k", "v")], axis=0)
        elif cfg.backbone == BACKBONE_T5 and ".DenseReluDense.Wgu." in n:       # T5DenseGatedActDense wi_0 / wi_1: rows wi_0 | wi_1
            out[n] = np.concatenate([find(n.replace("Wgu", part)) for part in ("wi_0", "wi_1")], axis=0)
        elif cfg.backbone == BACKBONE_T5 and n == "shared.weight":              # (a bare T5EncoderModel may store the tied copy only)
            try:
                out[n] = find(n)
            except KeyError:
                out[n] = find("encoder.embed_tokens.weight")
        else:
            out[n] = find(n)
    return out


# ---- BERT / RoBERTa / XLM-R checkpoints (mirrors parse_config of host/glc_safetensors.c) ----
BERT_MODEL_TYPES = ("bert", "roberta", "xlm-roberta")
_BERT_PREFIXES = ("bert.", "roberta.", "encoder_model.", "model.encoder_model.", "encoder_model.bert.", "encoder_model.roberta.",
                  "model.encoder_model.bert.", "model.encoder_model.roberta.")


def bert_config_from_hf(root: dict, vocab: int = None) -> GLiClassConfig:
    """GLiClassConfig of a BERT-family checkpoint's config.json (`root`; the backbone's own fields under encoder_config, or a bare
    backbone config).  `vocab` = rows of the word-embedding matrix (tokens were added after the backbone config was written).
    Everything the engine does not build is refused with a message that names the field."""
    from .config import SCORER_NAMES, POOL_FIRST, POOL_AVG, POOL_LAST
    enc = root.get("encoder_config") if isinstance(root.get("encoder_config"), dict) else root
    mt = enc.get("model_type")
    if mt not in BERT_MODEL_TYPES:
        raise ValueError(f"backbone model_type '{mt}' is not a BERT-family type (bert, roberta, xlm-roberta)")
    pet = enc.get("position_embedding_type", "absolute")
    if pet != "absolute":
        raise ValueError(f"position_embedding_type '{pet}' is not implemented (absolute)")
    act = enc.get("hidden_act", "gelu")
    if act != "gelu":
        raise ValueError(f"hidden_act '{act}' is not implemented (gelu)")
    if enc.get("is_decoder", False):
        raise ValueError("is_decoder=true is not implemented")
    if enc.get("add_cross_attention", False):
        raise ValueError("add_cross_attention=true is not implemented")
    H, nh = int(enc["hidden_size"]), int(enc["num_attention_heads"])
    if H % nh or H // nh != 64:
        raise ValueError(f"head_dim {H // nh} is not implemented (64)")
    pad = int(enc.get("pad_token_id", 0 if mt == "bert" else 1))
    off = 0 if mt == "bert" else pad + 1
    P = int(enc.get("max_position_embeddings", 512))
    if P - off < 1:
        raise ValueError(f"max_position_embeddings {P} leaves no position behind the offset {off}")
    pool = {"first": POOL_FIRST, "avg": POOL_AVG, "last": POOL_LAST}[root.get("pooling_strategy", "first")]
    vocab = int(vocab if vocab is not None else root.get("vocab_size", enc.get("vocab_size")))
    return GLiClassConfig(
        name="checkpoint", vocab=vocab, hidden=H, layers=int(enc["num_hidden_layers"]), heads=nh, inter=int(enc["intermediate_size"]),
        pos_buckets=0, max_rel_pos=0, ln_eps=float(enc.get("layer_norm_eps", 1e-12)), pad_id=pad,
        cls_id=int(enc.get("cls_token_id", enc.get("bos_token_id", 1))), sep_id=int(enc.get("sep_token_id", enc.get("eos_token_id", 2))),
        class_token_index=int(root.get("class_token_index", -1)), text_token_index=int(root.get("text_token_index", -1)), pooling=pool,
        scorer=SCORER_NAMES[root.get("scorer_type", "simple")], embed_class_token=int(bool(root.get("embed_class_token", True))),
        normalize_features=int(bool(root.get("normalize_features", False))), logit_scale=float(root.get("logit_scale", 1.0)),
        backbone=BACKBONE_BERT, causal=0, max_positions=P, type_vocab=int(enc.get("type_vocab_size", 2)), pos_offset=off)


def load_bert_checkpoint(path: str) -> Tuple[GLiClassConfig, Dict[str, np.ndarray]]:
    """An HF directory (config.json + model.safetensors) of a BERT-family backbone -> (config, tensors in blob order)."""
    import json
    import os
    from safetensors.numpy import load_file
    with open(os.path.join(path, "config.json")) as f:
        root = json.load(f)
    sd = load_file(os.path.join(path, "model.safetensors"))
    emb = [v for k, v in sd.items() if k.endswith("embeddings.word_embeddings.weight")]
    if not emb:
        raise KeyError("embeddings.word_embeddings.weight")
    cfg = bert_config_from_hf(root, vocab=emb[0].shape[0])
    return cfg, from_state_dict(sd, cfg)


# ---- T5 / mT5 checkpoints (mirrors parse_config of host/glc_safetensors.c) ----
T5_MODEL_TYPES = ("t5", "mt5")


def t5_config_from_hf(root: dict, vocab: int = None) -> GLiClassConfig:
    """GLiClassConfig of a T5-family checkpoint's config.json (`root`; the backbone's own fields under encoder_config, or a bare
    backbone config).  `vocab` = rows of the shared embedding.  Everything the engine does not build is refused with a message that
    names the field."""
    from .config import SCORER_NAMES, POOL_FIRST, POOL_AVG, POOL_LAST
    enc = root.get("encoder_config") if isinstance(root.get("encoder_config"), dict) else root
    mt = enc.get("model_type")
    if mt == "umt5":
        raise ValueError("model_type 'umt5' is not implemented (a relative_attention_bias table per layer; t5 and mt5 share layer 0's)")
    if mt not in T5_MODEL_TYPES:
        raise ValueError(f"backbone model_type '{mt}' is not a T5-family type (t5, mt5)")
    ffp = enc.get("feed_forward_proj", "relu")
    if ffp != "gated-gelu":
        raise ValueError(f"feed_forward_proj '{ffp}' is not implemented (gated-gelu)")
    act = enc.get("dense_act_fn", "gelu_new")
    if act != "gelu_new":
        raise ValueError(f"dense_act_fn '{act}' is not implemented (gelu_new)")
    dkv = int(enc.get("d_kv", 64))
    if dkv != 64:
        raise ValueError(f"d_kv {dkv} is not implemented (64)")
    if enc.get("is_decoder", False):
        raise ValueError("is_decoder=true is not implemented")
    nb, md = int(enc.get("relative_attention_num_buckets", 32)), int(enc.get("relative_attention_max_distance", 128))
    if nb < 4 or nb % 4 or md <= nb // 4:
        raise ValueError(f"relative_attention_num_buckets {nb} / relative_attention_max_distance {md} is not implemented "
                         "(a multiple of 4, max distance beyond a quarter of it)")
    pool = {"first": POOL_FIRST, "avg": POOL_AVG, "last": POOL_LAST}[root.get("pooling_strategy", "first")]
    vocab = int(vocab if vocab is not None else root.get("vocab_size", enc.get("vocab_size")))
    return GLiClassConfig(
        name="checkpoint", vocab=vocab, hidden=int(enc["d_model"]), layers=int(enc["num_layers"]), heads=int(enc["num_heads"]),
        inter=int(enc["d_ff"]), head_dim=64, pos_buckets=0, max_rel_pos=0, ln_eps=float(enc.get("layer_norm_epsilon", 1e-6)),
        pad_id=int(enc.get("pad_token_id", 0)), cls_id=int(enc.get("cls_token_id", enc.get("bos_token_id", 1)) or 1),
        sep_id=int(enc.get("sep_token_id", enc.get("eos_token_id", 2))),
        class_token_index=int(root.get("class_token_index", -1)), text_token_index=int(root.get("text_token_index", -1)), pooling=pool,
        scorer=SCORER_NAMES[root.get("scorer_type", "simple")], embed_class_token=int(bool(root.get("embed_class_token", True))),
        normalize_features=int(bool(root.get("normalize_features", False))), logit_scale=float(root.get("logit_scale", 1.0)),
        backbone=BACKBONE_T5, causal=0, rel_buckets=nb, rel_max_distance=md)


def load_t5_checkpoint(path: str) -> Tuple[GLiClassConfig, Dict[str, np.ndarray]]:
    """An HF directory (config.json + model.safetensors) of a T5-family backbone -> (config, tensors in blob order).  Decoder-side
    tensors are ignored; a checkpoint without encoder tensors is refused."""
    import json
    import os
    from safetensors.numpy import load_file
    with open(os.path.join(path, "config.json")) as f:
        root = json.load(f)
    cfg0 = t5_config_from_hf(root, vocab=1)                   # (the refusals, before the file is read)
    sd = load_file(os.path.join(path, "model.safetensors"))
    if not any(k.endswith("encoder.block.0.layer.0.SelfAttention.q.weight") for k in sd):
        raise ValueError("is_encoder_decoder: the checkpoint holds no encoder tensors (encoder.block.0.layer.0.SelfAttention.q.weight)")
    emb = [v for k, v in sd.items() if k.endswith("shared.weight") or k.endswith("encoder.embed_tokens.weight")]
    if not emb:
        raise KeyError("shared.weight")
    cfg = t5_config_from_hf(root, vocab=emb[0].shape[0])
    del cfg0
    return cfg, from_state_dict(sd, cfg)


# ---- *ForSequenceClassification checkpoints (head_kind = HEAD_SEQCLS; the arithmetic and its transformers sources: csrc/cls_head.hip) ----
SEQCLS_MODEL_TYPES = ("deberta-v2", "bert", "roberta", "xlm-roberta", "modernbert")
# checkpoint names of the six head slots (CLS_HEAD_NAMES order) per model_type; None = the class has no such tensor
_SEQCLS_HEAD_KEYS = {
    "deberta-v2": ("pooler.dense.weight", "pooler.dense.bias", None, None, "classifier.weight", "classifier.bias"),
    "bert": ("bert.pooler.dense.weight", "bert.pooler.dense.bias", None, None, "classifier.weight", "classifier.bias"),
    "roberta": ("classifier.dense.weight", "classifier.dense.bias", None, None, "classifier.out_proj.weight", "classifier.out_proj.bias"),
    "modernbert": ("head.dense.weight", "head.dense.bias", "head.norm.weight", "head.norm.bias", "classifier.weight", "classifier.bias"),
}
_SEQCLS_HEAD_KEYS["xlm-roberta"] = _SEQCLS_HEAD_KEYS["roberta"]


def _num_labels(root: dict) -> int:
    if isinstance(root.get("id2label"), dict) and root["id2label"]:
        return len(root["id2label"])
    return int(root.get("num_labels", 2))


def seqcls_config_from_hf(root: dict, vocab: int = None) -> GLiClassConfig:
    """GLiClassConfig of a *ForSequenceClassification checkpoint's config.json (a bare HF config: `architectures` names the class, the backbone's
    fields lie at the top level).  The backbone fields go through the same checks as the GLiClass importers'; everything the engine does not
    build is refused with a message that names the field.  Mirrors the sequence-classification block at the end of parse_config in
    host/glc_safetensors.c."""
    import dataclasses
    arch = root.get("architectures") or []
    if not any(str(a).endswith("ForSequenceClassification") for a in arch):
        raise ValueError(f"architectures {arch} names no *ForSequenceClassification class")
    mt = root.get("model_type")
    if mt not in SEQCLS_MODEL_TYPES:
        raise ValueError(f"model_type '{mt}' has no sequence-classification head in this engine ({', '.join(SEQCLS_MODEL_TYPES)}; decoder and T5 "
                         "classes are out of scope)")
    K = _num_labels(root)
    if not 1 <= K <= CLS_MAX_LABELS:
        raise ValueError(f"num_labels {K} is not implemented (1 .. {CLS_MAX_LABELS})")
    # (a bare HF config: no GLiClass wrapper keys; a key HF wrote as null counts as absent)
    bare = {k: v for k, v in root.items() if v is not None and k not in ("class_token_index", "text_token_index", "scorer_type", "pooling_strategy", "encoder_config")}
    if mt in BERT_MODEL_TYPES:
        base = bert_config_from_hf(bare, vocab=vocab)
        head = dict(pooling=POOL_FIRST, cls_act=CLS_ACT_TANH, cls_norm=0, cls_dense=1)
    elif mt == "modernbert":
        base = modernbert_config_from_hf(bare, vocab=vocab)
        act = root.get("classifier_activation", "gelu")
        if act != "gelu":
            raise ValueError(f"classifier_activation '{act}' is not implemented (gelu)")
        cp = root.get("classifier_pooling", "cls")
        if cp not in ("cls", "mean"):
            raise ValueError(f"classifier_pooling '{cp}' is not implemented (cls, mean)")
        head = dict(pooling=POOL_FIRST if cp == "cls" else POOL_AVG, cls_act=CLS_ACT_GELU, cls_norm=1, cls_dense=1)
    else:
        base = deberta_config_from_hf(bare, vocab=vocab)
        phs = int(root.get("pooler_hidden_size", base.hidden))
        if phs != base.hidden:
            raise ValueError(f"pooler_hidden_size {phs} != hidden_size {base.hidden} is not implemented")
        act = root.get("pooler_hidden_act", "gelu")
        if act != "gelu":
            raise ValueError(f"pooler_hidden_act '{act}' is not implemented (gelu)")
        head = dict(pooling=POOL_FIRST, cls_act=CLS_ACT_GELU, cls_norm=0, cls_dense=1)
    return dataclasses.replace(base, head_kind=HEAD_SEQCLS, cls_labels=K, **head)


def deberta_config_from_hf(root: dict, vocab: int = None) -> GLiClassConfig:
    """GLiClassConfig of a bare DebertaV2Config (deberta-v2 / deberta-v3 checkpoints): the disentangled-attention settings every published
    deberta-v3 has; everything else is refused with a message that names the field.  Mirrors the "deberta-v2" branch of parse_config in
    host/glc_safetensors.c, field for field; tests/test_seqcls_host.py::test_c_reader_and_python_importer_agree and
    ::test_importer_refusals_name_the_field run both on the same checkpoints and the same refused fields."""
    if root.get("model_type") != "deberta-v2":
        raise ValueError(f"model_type '{root.get('model_type')}' is not deberta-v2")
    if not root.get("relative_attention", False):
        raise ValueError("relative_attention=false is not implemented (true)")
    pat = root.get("pos_att_type") or []
    pat = pat.split("|") if isinstance(pat, str) else list(pat)
    if sorted(pat) != ["c2p", "p2c"]:
        raise ValueError(f"pos_att_type {pat} is not implemented (p2c|c2p)")
    if not root.get("share_att_key", False):
        raise ValueError("share_att_key=false is not implemented (true)")
    if "layer_norm" not in str(root.get("norm_rel_ebd", "none")):
        raise ValueError(f"norm_rel_ebd '{root.get('norm_rel_ebd')}' is not implemented (layer_norm)")
    if root.get("position_biased_input", True):
        raise ValueError("position_biased_input=true is not implemented (false)")
    if int(root.get("conv_kernel_size", 0) or 0) > 0:
        raise ValueError(f"conv_kernel_size {root.get('conv_kernel_size')} is not implemented (0)")
    if int(root.get("type_vocab_size", 0) or 0) > 0:
        raise ValueError(f"type_vocab_size {root.get('type_vocab_size')} is not implemented (0)")
    if int(root.get("embedding_size", root["hidden_size"])) != int(root["hidden_size"]):
        raise ValueError(f"embedding_size {root.get('embedding_size')} != hidden_size is not implemented")
    act = root.get("hidden_act", "gelu")
    if act != "gelu":
        raise ValueError(f"hidden_act '{act}' is not implemented (gelu)")
    H, nh = int(root["hidden_size"]), int(root["num_attention_heads"])
    if H % nh or H // nh != 64:
        raise ValueError(f"head_dim {H // nh} is not implemented (64)")
    mrp = int(root.get("max_relative_positions", -1))
    if mrp < 1:
        mrp = int(root.get("max_position_embeddings", 512))
    vocab = int(vocab if vocab is not None else root["vocab_size"])
    return GLiClassConfig(name="checkpoint", vocab=vocab, hidden=H, layers=int(root["num_hidden_layers"]), heads=nh, inter=int(root["intermediate_size"]),
                          pos_buckets=int(root.get("position_buckets", -1)) if int(root.get("position_buckets", -1)) > 0 else 0, max_rel_pos=mrp,
                          ln_eps=float(root.get("layer_norm_eps", 1e-7)), pad_id=int(root.get("pad_token_id", 0)),
                          cls_id=int(root.get("cls_token_id", root.get("bos_token_id", 1)) or 1), sep_id=int(root.get("sep_token_id", root.get("eos_token_id", 2)) or 2),
                          backbone=BACKBONE_DEBERTA)


def modernbert_config_from_hf(root: dict, vocab: int = None) -> GLiClassConfig:
    """GLiClassConfig of a bare ModernBertConfig; everything the engine does not build is refused with a message that names the field.
    Mirrors the "modernbert" branch of parse_config in host/glc_safetensors.c (both forms of the configuration), held to it by the same
    two tests as deberta_config_from_hf."""
    if root.get("model_type") != "modernbert":
        raise ValueError(f"model_type '{root.get('model_type')}' is not modernbert")
    for f in ("attention_bias", "mlp_bias", "norm_bias"):
        if root.get(f, False):
            raise ValueError(f"{f}=true is not implemented (false)")
    act = root.get("hidden_activation", "gelu")
    if act != "gelu":
        raise ValueError(f"hidden_activation '{act}' is not implemented (gelu)")
    H, nh = int(root["hidden_size"]), int(root["num_attention_heads"])
    if H % nh or H // nh != 64:
        raise ValueError(f"head_dim {H // nh} is not implemented (64)")
    la = int(root.get("local_attention", 128))
    if la < 0 or la % 2:
        raise ValueError(f"local_attention {la} is not implemented (an even window)")
    # (both forms of configuration_modernbert.py: global_attn_every_n_layers / global_rope_theta / local_rope_theta, or layer_types / rope_parameters)
    L = int(root["num_hidden_layers"])
    every = int(root.get("global_attn_every_n_layers", 3))
    lt = root.get("layer_types")
    if isinstance(lt, list):
        if len(lt) != L or any(t not in ("full_attention", "sliding_attention") for t in lt):
            raise ValueError("layer_types must name 'full_attention' or 'sliding_attention' for every layer")
        full = [l for l in range(1, L) if lt[l] == "full_attention"]
        every = full[0] if full else max(L, 1)
        if any((lt[l] == "full_attention") != (l % every == 0) for l in range(L)):
            raise ValueError("layer_types is not periodic (full attention on every n-th layer from layer 0)")
    theta_g, theta_l = float(root.get("global_rope_theta", 160000.0)), float(root.get("local_rope_theta") or 10000.0)
    rp = root.get("rope_parameters")
    if isinstance(rp, dict):
        for key in ("full_attention", "sliding_attention"):
            if isinstance(rp.get(key), dict) and rp[key].get("rope_type", "default") != "default":
                raise ValueError(f"rope_parameters.{key}.rope_type '{rp[key]['rope_type']}' is not implemented (default)")
        theta_g = float((rp.get("full_attention") or {}).get("rope_theta", theta_g))
        theta_l = float((rp.get("sliding_attention") or {}).get("rope_theta", theta_l))
    vocab = int(vocab if vocab is not None else root["vocab_size"])
    return GLiClassConfig(name="checkpoint", vocab=vocab, hidden=H, layers=int(root["num_hidden_layers"]), heads=nh, inter=int(root["intermediate_size"]),
                          pos_buckets=0, max_rel_pos=0, ln_eps=float(root.get("norm_eps", 1e-5)), pad_id=int(root.get("pad_token_id", 50283)),
                          cls_id=int(root.get("cls_token_id", root.get("bos_token_id", 50281))), sep_id=int(root.get("sep_token_id", root.get("eos_token_id", 50282))),
                          backbone=BACKBONE_MODERNBERT, causal=0, rope_theta=theta_g, local_window=la // 2, global_every=every, rope_theta_local=theta_l)


def seqcls_from_state_dict(sd: Dict[str, "np.ndarray"], cfg: GLiClassConfig, model_type: str) -> Dict[str, np.ndarray]:
    """Backbone tensors under their blob names (from_state_dict: the prefixes `deberta.`, `bert.`, `roberta.`, `model.`) + the head's six slots;
    a head tensor the class does not have, or has switched off, is left out."""
    names = [n for n, _, _, _ in tensor_specs(cfg) if not n.startswith("cls.")]
    out = from_state_dict(sd, cfg, names=names)
    for blob_name, key in zip(CLS_HEAD_NAMES, _SEQCLS_HEAD_KEYS[model_type]):
        if key is None or key not in sd:
            if blob_name in CLS_OPTIONAL_BIASES or key is None:
                continue
            raise KeyError(key)
        v = sd[key]
        out[blob_name] = v.detach().cpu().float().numpy() if hasattr(v, "detach") else np.asarray(v, np.float32)
    return out


def load_seqcls_checkpoint(path: str) -> Tuple[GLiClassConfig, Dict[str, np.ndarray]]:
    """An HF directory (config.json + model.safetensors) saved by a DebertaV2 / Bert / Roberta / XLMRoberta / ModernBert
    ForSequenceClassification model -> (config with head_kind = HEAD_SEQCLS, tensors under blob names).  No GLiClass wrapper keys and no
    <<LABEL>> / <<SEP>> vocabulary rows are expected."""
    import json
    import os
    from safetensors.numpy import load_file
    with open(os.path.join(path, "config.json")) as f:
        root = json.load(f)
    seqcls_config_from_hf(root, vocab=1)                      # (the refusals, before the file is read)
    sd = load_file(os.path.join(path, "model.safetensors"))
    emb = [v for k, v in sd.items() if k.endswith("embeddings.word_embeddings.weight") or k.endswith("embeddings.tok_embeddings.weight")]
    if not emb:
        raise KeyError("embeddings.word_embeddings.weight")
    cfg = seqcls_config_from_hf(root, vocab=emb[0].shape[0])
    return cfg, seqcls_from_state_dict(sd, cfg, root["model_type"])
