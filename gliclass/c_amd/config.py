"""Model configurations for the GLiClass hot path (encoder backbone, and the decoder backbone of BASELINE.json configs[4]).

The reference repo never states backbone dimensions (they live in the HF hub
`config.json` that `/root/reference/run_GLiClass.sh:34-36` downloads at run time);
the values below are the standard DeBERTa-v3 shapes listed in SURVEY.md §8a.
Every field is carried in the weight-blob header (`weights.py`), so a real
checkpoint overrides them — nothing here is a compile-time constant of the engine.
"""
from dataclasses import dataclass, asdict

# scorer / pooling enums shared with include/gliclass_hip.h
POOL_FIRST, POOL_AVG, POOL_LAST = 0, 1, 2
SCORER_DOT = 0
SCORER_WEIGHTED_DOT = 1
SCORER_MLP = 2
SCORER_MLP_HIDDEN = 256
SCORER_NAMES = {"simple": SCORER_DOT, "weighted-dot": SCORER_WEIGHTED_DOT, "mlp": SCORER_MLP}
BACKBONE_DEBERTA, BACKBONE_DECODER, BACKBONE_MODERNBERT, BACKBONE_BERT, BACKBONE_T5 = 0, 1, 2, 3, 4
HEAD_GLICLASS, HEAD_SEQCLS = 0, 1
CLS_ACT_NONE, CLS_ACT_TANH, CLS_ACT_GELU = 0, 1, 2
CLS_MAX_LABELS = 1024


@dataclass(frozen=True)
class GLiClassConfig:
    name: str
    vocab: int
    hidden: int
    layers: int
    heads: int
    inter: int
    head_dim: int = 64
    pos_buckets: int = 256          # DebertaV2Config.position_buckets
    max_rel_pos: int = 512          # max_relative_positions (= max_position_embeddings)
    ln_eps: float = 1e-7
    pad_id: int = 0
    cls_id: int = 1
    sep_id: int = 2
    class_token_index: int = -1     # id of "<<LABEL>>"   (/root/reference/src/preprocessor.c:68)
    text_token_index: int = -1      # id of "<<SEP>>"     (/root/reference/src/preprocessor.c:69)
    pooling: int = POOL_FIRST
    scorer: int = SCORER_DOT
    embed_class_token: int = 1
    normalize_features: int = 0
    logit_scale: float = 1.0
    # decoder-style backbone (Qwen2 arithmetic — RMSNorm, RoPE, grouped-query attention, SwiGLU);
    # ln_eps doubles as rms_norm_eps, `inter` is the SwiGLU width
    backbone: int = BACKBONE_DEBERTA
    kv_heads: int = 0               # 0 => heads (no grouping)
    causal: int = 1                 # BASELINE.json says causal; upstream may wrap decoders bidirectionally (unpinned) -> flag
    rope_theta: float = 1.0e6
    # ModernBERT backbone (transformers models/modernbert): rope_theta is the global layers' base, rope_theta_local the local
    # layers'; a local layer attends to keys with |q - k| <= local_window (= local_attention // 2; 0 = every layer global);
    # layer l is global when l % global_every == 0; ln_eps is norm_eps, `inter` the GeGLU width
    local_window: int = 0
    global_every: int = 1
    rope_theta_local: float = 1.0e4
    # decoder backbone: qk_norm = 1 is Qwen3's RMSNorm over head_dim on every query and key head before RoPE (gains q_norm / k_norm,
    # epsilon ln_eps); attn_bias = 0 drops the q / k / v projection biases (Llama, Qwen3).  Qwen2 is (0, 1).
    qk_norm: int = 0
    attn_bias: int = 1
    # BERT backbone (transformers models/bert, models/roberta, models/xlm_roberta): rows of the learned position table and of the token-type
    # table (row 0 is the only one used); pos_offset = 0 numbers positions 0 .. S-1 (BERT), pos_offset = pad_id + 1 numbers the non-pad
    # tokens from pos_offset on and gives pad tokens row pad_id (RoBERTa / XLM-R).  At most max_positions - pos_offset tokens per row.
    max_positions: int = 0
    type_vocab: int = 0
    pos_offset: int = 0
    # T5 backbone (transformers models/t5, the encoder stack): relative_attention_num_buckets / relative_attention_max_distance of the
    # learned bias table [rel_buckets, heads] (layer 0's, shared by all layers); head_dim is d_kv = 64, heads * head_dim need not be
    # `hidden` (mt5-small: 6 x 64 on 512); ln_eps is layer_norm_epsilon, `inter` d_ff (the gated-gelu width)
    rel_buckets: int = 0
    rel_max_distance: int = 0
    # head_kind = HEAD_SEQCLS: the head of an HF *ForSequenceClassification checkpoint in place of the GLiClass head (DeBERTa, BERT / RoBERTa /
    # XLM-R and ModernBERT backbones): pooled row (`pooling` first / avg) -> [dense H x H] -> cls_act (0 none, 1 tanh, 2 erf-GELU) ->
    # [LayerNorm, epsilon ln_eps] -> classifier with cls_labels outputs.  All 0 with the GLiClass head.
    head_kind: int = HEAD_GLICLASS
    cls_labels: int = 0
    cls_act: int = CLS_ACT_NONE
    cls_norm: int = 0
    cls_dense: int = 0

    def __post_init__(self):
        if self.head_kind == HEAD_SEQCLS:
            assert 1 <= self.cls_labels <= CLS_MAX_LABELS and self.cls_act in (0, 1, 2) and self.cls_norm in (0, 1) and self.cls_dense in (0, 1)
            assert self.pooling in (POOL_FIRST, POOL_AVG)
        else:
            assert self.head_kind == HEAD_GLICLASS and (self.cls_labels, self.cls_act, self.cls_norm, self.cls_dense) == (0, 0, 0, 0)
        # (a decoder checkpoint names its head_dim: Qwen3's is not hidden / heads; T5's inner width is num_heads * d_kv)
        assert self.backbone in (BACKBONE_DECODER, BACKBONE_T5) or self.hidden == self.heads * self.head_dim
        assert self.qk_norm in (0, 1) and self.attn_bias in (0, 1) and (self.backbone == BACKBONE_DECODER or self.qk_norm == 0)
        if self.kv_heads <= 0:
            object.__setattr__(self, "kv_heads", self.heads)
        assert self.heads % self.kv_heads == 0
        if self.backbone == BACKBONE_BERT:
            assert self.head_dim == 64 and self.type_vocab >= 1 and self.pos_offset in (0, self.pad_id + 1)
            assert self.max_positions - self.pos_offset >= 1
        if self.backbone == BACKBONE_T5:
            assert self.head_dim == 64 and self.rel_buckets >= 4 and self.rel_buckets % 4 == 0 and self.rel_max_distance > self.rel_buckets // 4
        if self.class_token_index < 0:
            object.__setattr__(self, "class_token_index", self.vocab - 2)
        if self.text_token_index < 0:
            object.__setattr__(self, "text_token_index", self.vocab - 1)

    @property
    def att_span(self) -> int:
        return self.pos_buckets if self.pos_buckets > 0 else self.max_rel_pos

    def flops_per_seq(self, S: int, C: int) -> float:
        """F_seq = L*S*(8H^2 + 4HI + 4SH + 4PH) + 8H^2(1+C); decoder:
        L*S*(4H*nq*d + 4H*nkv*d + 6HI + 4S*nq*d*kappa) + head, kappa = 1/2 when causal; ModernBERT:
        L*S*(8H^2 + 6HI) + sum_l 4*S*H*keys_l + head, keys_l = S on global layers and min(S, 2W+1) on local ones."""
        H, I, L, P = self.hidden, self.inter, self.layers, 2 * self.att_span
        if self.backbone == BACKBONE_BERT:          # the DeBERTa count without its position projections
            return L * S * (8 * H * H + 4 * H * I + 4 * S * H) + 8 * H * H * (1 + C)
        if self.backbone == BACKBONE_T5:            # the decoder count with nq = nkv = heads and full (bidirectional) attention
            nqd = self.heads * self.head_dim
            return L * S * (8 * H * nqd + 6 * H * I + 4 * S * nqd) + 8 * H * H * (1 + C)
        if self.backbone == BACKBONE_MODERNBERT:
            keys = sum(S if self.is_global_layer(l) else min(S, 2 * self.local_window + 1) for l in range(L))
            return L * S * (8 * H * H + 6 * H * I) + 4 * S * H * keys + 8 * H * H * (1 + C)
        if self.backbone == BACKBONE_DECODER:
            nqd, nkvd, kappa = self.heads * self.head_dim, self.kv_heads * self.head_dim, (0.5 if self.causal else 1.0)
            return L * S * (4 * H * nqd + 4 * H * nkvd + 6 * H * I + 4 * S * nqd * kappa) + 8 * H * H * (1 + C)
        return L * S * (8 * H * H + 4 * H * I + 4 * S * H + 4 * P * H) + 8 * H * H * (1 + C)

    def is_global_layer(self, l: int) -> bool:
        """ModernBERT: full attention (and the global RoPE base) on layer l."""
        return self.local_window <= 0 or l % max(self.global_every, 1) == 0

    def asdict(self):
        return asdict(self)


CONFIGS = {
    # parity-fixture config: real head_dim (64) and real bucket geometry (256/512) so the
    # clamp / log-bucket paths are exercised, everything else tiny.
    "tiny": GLiClassConfig("tiny", vocab=515, hidden=128, layers=2, heads=2, inter=256),
    "mini": GLiClassConfig("mini", vocab=1027, hidden=256, layers=3, heads=4, inter=512),
    "small": GLiClassConfig("small", vocab=128003, hidden=768, layers=6, heads=12, inter=3072),
    "base": GLiClassConfig("base", vocab=128003, hidden=768, layers=12, heads=12, inter=3072),
    "large": GLiClassConfig("large", vocab=128003, hidden=1024, layers=24, heads=16, inter=4096),
    # decoder-style backbones: real head_dim (128) and grouping; dec-tiny/dec-mini are the parity-fixture configs,
    # qwen-1.5b is BASELINE.json configs[4] (Qwen2-1.5B shape; vocab 151 646 + <<LABEL>>, <<SEP>>)
    "dec-tiny": GLiClassConfig("dec-tiny", vocab=515, hidden=256, layers=2, heads=2, inter=512, head_dim=128, kv_heads=1,
                               ln_eps=1e-6, backbone=BACKBONE_DECODER, pooling=POOL_LAST),
    "dec-mini": GLiClassConfig("dec-mini", vocab=1027, hidden=512, layers=3, heads=4, inter=768, head_dim=128, kv_heads=2,
                               ln_eps=1e-6, backbone=BACKBONE_DECODER, pooling=POOL_LAST),
    "qwen-1.5b": GLiClassConfig("qwen-1.5b", vocab=151648, hidden=1536, layers=28, heads=12, inter=8960, head_dim=128,
                                kv_heads=2, ln_eps=1e-6, backbone=BACKBONE_DECODER, pooling=POOL_LAST),
    # Qwen3 arithmetic (per-head QK RMSNorm, no projection biases): q3-tiny (head_dim 64, H % 256 != 0: the plain paths, nq d = H) and
    # q3-mini (head_dim 128, nq d = 512 != H, group-split eligible) are the parity-fixture configs, qwen3-0.6b the published shape
    # (vocab 151 936 + <<LABEL>>, <<SEP>>); ll-tiny is dec-tiny with Llama arithmetic (no biases, no QK norm)
    "q3-tiny": GLiClassConfig("q3-tiny", vocab=515, hidden=128, layers=2, heads=2, inter=256, head_dim=64, kv_heads=1, ln_eps=1e-6,
                              backbone=BACKBONE_DECODER, pooling=POOL_LAST, qk_norm=1, attn_bias=0),
    "q3-mini": GLiClassConfig("q3-mini", vocab=1027, hidden=256, layers=3, heads=4, inter=768, head_dim=128, kv_heads=2, ln_eps=1e-6,
                              backbone=BACKBONE_DECODER, pooling=POOL_LAST, qk_norm=1, attn_bias=0),
    "ll-tiny": GLiClassConfig("ll-tiny", vocab=515, hidden=256, layers=2, heads=2, inter=512, head_dim=128, kv_heads=1, ln_eps=1e-6,
                              backbone=BACKBONE_DECODER, pooling=POOL_LAST, qk_norm=0, attn_bias=0),
    "qwen3-0.6b": GLiClassConfig("qwen3-0.6b", vocab=151938, hidden=1024, layers=28, heads=16, inter=3072, head_dim=128, kv_heads=8,
                                 ln_eps=1e-6, backbone=BACKBONE_DECODER, pooling=POOL_LAST, qk_norm=1, attn_bias=0),
    # ModernBERT backbones: mb-tiny / mb-mini are the parity-fixture configs (mb-tiny: H % 256 != 0, the paths without group split;
    # mb-mini: group-split eligible), modernbert-base / -large the published shapes (vocab 50 368 + <<LABEL>>, <<SEP>>)
    "mb-tiny": GLiClassConfig("mb-tiny", vocab=515, hidden=128, layers=4, heads=2, inter=192, ln_eps=1e-5, backbone=BACKBONE_MODERNBERT,
                              causal=0, rope_theta=160000.0, local_window=8, global_every=3, rope_theta_local=10000.0),
    "mb-mini": GLiClassConfig("mb-mini", vocab=1027, hidden=256, layers=4, heads=4, inter=384, ln_eps=1e-5, backbone=BACKBONE_MODERNBERT,
                              causal=0, rope_theta=160000.0, local_window=64, global_every=3, rope_theta_local=10000.0, pooling=POOL_AVG),
    "modernbert-base": GLiClassConfig("modernbert-base", vocab=50370, hidden=768, layers=22, heads=12, inter=1152, ln_eps=1e-5,
                                      backbone=BACKBONE_MODERNBERT, causal=0, rope_theta=160000.0, local_window=64, global_every=3,
                                      rope_theta_local=10000.0),
    "modernbert-large": GLiClassConfig("modernbert-large", vocab=50370, hidden=1024, layers=28, heads=16, inter=2624, ln_eps=1e-5,
                                       backbone=BACKBONE_MODERNBERT, causal=0, rope_theta=160000.0, local_window=64, global_every=3,
                                       rope_theta_local=10000.0),
    # BERT / RoBERTa / XLM-R backbones: bert-tiny (RoBERTa position ids; H % 256 != 0: the plain paths) and bert-mini (group-split eligible;
    # a 2050-row position table, one token type) are the parity configs, bert-base the published BERT shape (vocab 30 522)
    "bert-tiny": GLiClassConfig("bert-tiny", vocab=515, hidden=128, layers=3, heads=2, inter=512, ln_eps=1e-5, pad_id=1, cls_id=0,
                                backbone=BACKBONE_BERT, causal=0, max_positions=514, type_vocab=2, pos_offset=2),
    "bert-mini": GLiClassConfig("bert-mini", vocab=1027, hidden=256, layers=4, heads=4, inter=1024, ln_eps=1e-5, pad_id=1, cls_id=0,
                                backbone=BACKBONE_BERT, causal=0, max_positions=2050, type_vocab=1, pos_offset=2),
    "bert-base": GLiClassConfig("bert-base", vocab=30522, hidden=768, layers=12, heads=12, inter=3072, ln_eps=1e-12, pad_id=0, cls_id=101,
                                sep_id=102, backbone=BACKBONE_BERT, causal=0, max_positions=512, type_vocab=2, pos_offset=0),
    # T5 v1.1 / mT5 backbones (gated-gelu, 32 buckets up to distance 128): t5-tiny (H % 256 != 0: the plain paths), t5-odd (3 heads: inner
    # width 192 != hidden, and an odd head count) and t5-mini (group-split eligible) are the parity configs, t5-base the published
    # T5 v1.1 base shape (vocab 32 128)
    "t5-tiny": GLiClassConfig("t5-tiny", vocab=515, hidden=128, layers=2, heads=2, inter=256, ln_eps=1e-6, backbone=BACKBONE_T5, causal=0,
                              pos_buckets=0, max_rel_pos=0, rel_buckets=32, rel_max_distance=128),
    "t5-odd": GLiClassConfig("t5-odd", vocab=515, hidden=128, layers=2, heads=3, inter=256, ln_eps=1e-6, backbone=BACKBONE_T5, causal=0,
                             pos_buckets=0, max_rel_pos=0, rel_buckets=32, rel_max_distance=128),
    "t5-mini": GLiClassConfig("t5-mini", vocab=1027, hidden=256, layers=3, heads=4, inter=512, ln_eps=1e-6, backbone=BACKBONE_T5, causal=0,
                              pos_buckets=0, max_rel_pos=0, rel_buckets=32, rel_max_distance=128),
    "t5-base": GLiClassConfig("t5-base", vocab=32128, hidden=768, layers=12, heads=12, inter=2048, ln_eps=1e-6, backbone=BACKBONE_T5, causal=0,
                              pos_buckets=0, max_rel_pos=0, rel_buckets=32, rel_max_distance=128),
}
