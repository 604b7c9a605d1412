"""Thin Python handle over the HIP engine C-ABI (tests, bench.py, smoke).  All compute happens in
libgliclass_hip.so; this module only marshals numpy buffers."""
import ctypes as C
import dataclasses

import numpy as np

from . import _lib
from .config import GLiClassConfig, HEAD_SEQCLS
from .weights import tensor_specs, CLS_HEAD_NAMES, CLS_OPTIONAL_BIASES

DTYPES = {"f32": 0, "bf16": 1, "f16": 2}
DTYPE_NAMES = {v: k for k, v in DTYPES.items()}


def to_c_config(cfg: GLiClassConfig) -> _lib.ModelConfig:
    return _lib.ModelConfig(cfg.vocab, cfg.hidden, cfg.layers, cfg.heads, cfg.head_dim, cfg.inter, cfg.pos_buckets,
                            cfg.max_rel_pos, cfg.pad_id, cfg.cls_id, cfg.sep_id, cfg.class_token_index, cfg.text_token_index,
                            cfg.pooling, cfg.scorer, cfg.embed_class_token, cfg.normalize_features, cfg.backbone, cfg.kv_heads,
                            cfg.causal, cfg.ln_eps, cfg.logit_scale, cfg.rope_theta, cfg.local_window, cfg.global_every,
                            cfg.rope_theta_local, cfg.qk_norm, cfg.attn_bias, cfg.max_positions, cfg.type_vocab, cfg.pos_offset,
                            cfg.rel_buckets, cfg.rel_max_distance, cfg.head_kind, cfg.cls_labels, cfg.cls_act, cfg.cls_norm, cfg.cls_dense)


def delta_table(S, bucket_size=256, max_position=512):
    out = np.zeros(2 * S - 1, np.int32)
    _lib.hip().glc_delta_table(S, bucket_size, max_position, out.ctypes.data)
    return out


def t5_bucket_table(S, num_buckets=32, max_distance=128):
    """T5's bidirectional relative-position bucket of delta = key - query for delta in [-(S-1), S-1] (host function of the engine library)"""
    out = np.zeros(2 * S - 1, np.int32)
    _lib.hip().glc_t5_bucket_table(S, num_buckets, max_distance, out.ctypes.data)
    return out


class Engine:
    def __init__(self, cfg: GLiClassConfig, tensors, dtype="f32", device=0):
        self.L = _lib.hip()
        self.cfg = cfg
        self.dtype = dtype
        if cfg.head_kind == HEAD_SEQCLS:
            # the six head slots of the C-ABI; a tensor the checkpoint does not have (no dense stage, no norm, a bias switched off) is a null pointer
            names = [s[0] for s in tensor_specs(dataclasses.replace(cfg, cls_dense=1, cls_norm=1))]
            have = {s[0] for s in tensor_specs(cfg)}
            absent = {n for n in CLS_HEAD_NAMES if n not in have or (n in CLS_OPTIONAL_BIASES and tensors.get(n) is None)}
        else:
            names, absent = [s[0] for s in tensor_specs(cfg)], set()
        arrs = [None if n in absent else np.ascontiguousarray(tensors[n], np.float32) for n in names]
        ptrs = (C.c_void_p * len(arrs))(*[None if a is None else a.ctypes.data for a in arrs])
        cc = to_c_config(cfg)
        self.h = self.L.glc_engine_create(C.byref(cc), ptrs, len(arrs), device, DTYPES[dtype])
        if not self.h:
            raise RuntimeError("glc_engine_create: " + self.L.glc_last_error().decode())

    @classmethod
    def from_spec(cls, cfg: GLiClassConfig, spec: str, dtype="f32", device=0):
        """Engine from a model path / "synthetic:<config>[:seed]" through the C weight source (glc_weights_load, the same
        code create_ort_session uses) — no Python-side copy of the tensors, which matters for the 1.5 B-parameter config."""
        M = _lib.model()
        w = _lib.Weights()
        if M.glc_weights_load(spec.encode(), C.byref(w)) != 0:
            raise RuntimeError(f"glc_weights_load({spec}) failed")
        self = cls.__new__(cls)
        self.L = _lib.hip()
        self.cfg = cfg
        self.dtype = dtype
        try:
            self.h = self.L.glc_engine_create(C.byref(w.cfg), C.cast(w.tensors, C.POINTER(C.c_void_p)), w.n_tensors, device, DTYPES[dtype])
        finally:
            M.glc_weights_free(C.byref(w))
        if not self.h:
            raise RuntimeError("glc_engine_create: " + self.L.glc_last_error().decode())
        return self

    def close(self):
        if getattr(self, "h", None):
            self.L.glc_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _err(self, what):
        return RuntimeError(f"{what}: {self.L.glc_last_error().decode()}")

    def forward(self, ids, mask, c_alloc=None):
        ids = np.ascontiguousarray(ids, np.int64)
        mask = np.ascontiguousarray(mask, np.int64)
        B, S = ids.shape
        if c_alloc is None:
            c_alloc = self.cfg.cls_labels if self.cfg.head_kind == HEAD_SEQCLS else int((ids == self.cfg.class_token_index).sum(1).max())
        logits = np.zeros((B, max(c_alloc, 1)), np.float32)
        c_out = C.c_int(0)
        if self.L.glc_engine_forward(self.h, ids.ctypes.data, mask.ctypes.data, B, S, logits.ctypes.data, c_alloc, C.byref(c_out)) != 0:
            raise self._err("glc_engine_forward")
        self.last_c = c_out.value
        return logits[:, :c_alloc]

    def num_labels(self):
        """width of the classifier output of a sequence-classification engine (head_kind 1); 0 with the GLiClass head"""
        return int(self.L.glc_engine_config(self.h).contents.cls_labels)

    def nli_scores(self, logits, T, Lb, entail_id, contra_id, multi_label=False):
        """zero-shot NLI: pair logits [T * Lb, K] (pair (t, l) in row t * Lb + l, as a forward of the pair batch returns them) -> probabilities
        [T, Lb] on the device, with the semantics of transformers' zero-shot pipeline: multi_label = the entailment share of softmax over
        (contradiction, entailment) per pair; else softmax of the entailment logits over a text's labels"""
        logits = np.ascontiguousarray(logits, np.float32)
        if logits.shape != (T * Lb, self.cfg.cls_labels):
            raise ValueError(f"nli_scores: logits {logits.shape}, expected {(T * Lb, self.cfg.cls_labels)}")
        out = np.zeros((T, Lb), np.float32)
        d_in, d_out = self.dev_alloc(max(logits.nbytes, 4)), self.dev_alloc(max(out.nbytes, 4))
        try:
            self.h2d(d_in, logits)
            if self.L.glc_engine_nli_scores(self.h, d_in, T, Lb, int(entail_id), int(contra_id), int(bool(multi_label)), d_out) != 0:
                raise self._err("glc_engine_nli_scores")
            self.sync()
            self.d2h(out, d_out)
        finally:
            self.dev_free(d_in)
            self.dev_free(d_out)
        return out

    def hidden(self, which, B, S):
        out = np.zeros((B, S, self.cfg.hidden), np.float32)
        if self.L.glc_debug_get_hidden(self.h, which, out.ctypes.data, out.size) != 0:
            raise self._err("glc_debug_get_hidden")
        return out

    def set_prune_last_layer(self, on=True):
        self.L.glc_engine_set_prune_last_layer(self.h, int(on))

    def last_pruned(self):
        """1: the last forward ran the compact (pruned) last layer, 0: it ran every row"""
        return int(self.L.glc_debug_last_forward_pruned(self.h))

    def set_length_buckets(self, max_groups):
        if self.L.glc_engine_set_length_buckets(self.h, int(max_groups)) != 0:
            raise self._err("glc_engine_set_length_buckets")

    def set_group_split(self, mode):
        """fp32 mode: 0 = plain fp32 activations + 128-tile split GEMMs, 1 = auto, 2 = group-split pipeline whenever the shapes allow"""
        if self.L.glc_debug_set_group_split(self.h, int(mode)) != 0:
            raise self._err("glc_debug_set_group_split")

    def last_group_split(self):
        return bool(self.L.glc_debug_last_forward_group_split(self.h))

    def last_ln_folded(self):
        return bool(self.L.glc_debug_last_forward_ln_folded(self.h))

    def set_ln_fused(self, on):
        """group-split pipeline: LayerNorm folded into the GEMMs around it (default) or as kernels of its own"""
        if self.L.glc_debug_set_ln_fused(self.h, int(bool(on))) != 0:
            raise self._err("glc_debug_set_ln_fused")

    def set_precision_mask(self, mask):
        """default mode, group-split pipeline: round operand groups to f16 (bits: include/gliclass_hip.h glc_debug_set_precision_mask)"""
        if self.L.glc_debug_set_precision_mask(self.h, int(mask)) != 0:
            raise self._err("glc_debug_set_precision_mask")

    def enable_mx(self):
        """ModernBERT backbone: build the GX weight copies and select the MX pipeline (opt-in there; raises with the condition that
        failed).  The other backbones take the pipeline by default: a no-op when it is available to the engine."""
        if self.L.glc_engine_enable_mx(self.h) != 0:
            raise self._err("glc_engine_enable_mx")

    def set_graph_replay(self, on=True):
        """captured-graph replay of forwards (opt-in): per shape and pipeline the first forward runs eagerly, the second is captured as a
        HIP graph, later ones are one launch; bit-identical results.  Off drops every cached graph."""
        if self.L.glc_engine_set_graph_replay(self.h, int(bool(on))) != 0:
            raise self._err("glc_engine_set_graph_replay")

    def last_graph(self):
        """the last forward: 0 ran eagerly, 1 was captured and launched, 2 replayed a cached graph (length-bucketed: the minimum over its groups)"""
        return int(self.L.glc_debug_last_forward_graph(self.h))

    def graph_cache_size(self):
        """graph executables the engine holds (at most 16)"""
        return int(self.L.glc_debug_graph_cache_size(self.h))

    def set_mx_small_forwards(self, mode):
        """DeBERTa backbone, fp32 mode (opt-in): MX pipeline for forwards below the 256 tile's fill rule, their small launches on the 128 tile of
        the MX GEMM.  0 = off, 1 = auto (the 128 tile's own fill rule), 2 = whenever the shapes allow.  Taken forwards move from ~1e-5 to the MX
        arithmetic's ~4e-5 against the oracle.  Raises on the other backbones for modes >= 1."""
        if self.L.glc_engine_set_mx_small_forwards(self.h, int(mode)) != 0:
            raise self._err("glc_engine_set_mx_small_forwards")

    def last_mx128(self):
        """GEMM launches of the last forward that ran on the 128 tile of the MX GEMM (0: none)"""
        return int(self.L.glc_debug_last_forward_mx128(self.h))

    def set_mx(self, on):
        """MX cross-term pipeline on / off (engine created under GLICLASS_MX=1 or =build)"""
        if self.L.glc_debug_set_mx(self.h, int(bool(on))) != 0:
            raise self._err("glc_debug_set_mx")

    def set_mx_attention(self, on):
        """MX pipeline: attention on MX tiles (default) or on split-f16 units"""
        self.L.glc_debug_set_mx_attention(self.h, int(bool(on)))

    def last_mx(self):
        return bool(self.L.glc_debug_last_forward_mx(self.h))

    def last_mx_attention(self):
        """the last forward's attention ran on MX tiles (attention_mx.hip)"""
        return bool(self.L.glc_debug_last_forward_mx_attention(self.h))

    def last_rope_epilogue(self):
        """decoder, MX pipeline: the last forward's QKV projections ran RoPE + MX tiles as their epilogue (never with qk_norm)"""
        return bool(self.L.glc_debug_last_forward_rope_epilogue(self.h))

    def fp8_range_retries(self):
        """host-buffer forwards repeated on the split-f16 kernels because an activation left the fp8 range of the MX operand images"""
        return int(self.L.glc_debug_fp8_range_retries(self.h))

    def fp8_range_sticky(self):
        """the engine has left the MX pipeline for good (outlier channels in consecutive forwards)"""
        return bool(self.L.glc_debug_fp8_range_sticky(self.h))

    def activation_exponent(self):
        """exponent of the MX pipeline's activation rows: 0, or -5 once a forward left the fp8 range (the guard's first answer)"""
        return int(self.L.glc_debug_activation_exponent(self.h))

    def range_retries(self):
        """host-buffer forwards repeated with the norms unfused because the folded forward came out non-finite"""
        return int(self.L.glc_debug_range_retries(self.h))

    def pos_ids(self, B, S):
        """BERT backbone: the position ids [B, Sp] of the last forward (Sp = S rounded up to 64), as the embedding kernel read them"""
        Sp = (S + 63) // 64 * 64
        out = np.zeros((B, Sp), np.int32)
        if self.L.glc_debug_read_pos_ids(self.h, out.ctypes.data, out.size) != 0:
            raise self._err("glc_debug_read_pos_ids")
        return out

    def keep_hidden(self, on=True):
        self.L.glc_debug_keep_hidden(self.h, int(on))

    def set_attention_impl(self, impl):
        if self.L.glc_debug_set_attention_impl(self.h, impl) != 0:
            raise self._err("glc_debug_set_attention_impl")

    # ---- device-resident path (bench) ----
    def dev_alloc(self, nbytes):
        p = self.L.glc_device_malloc(self.h, nbytes)
        if not p:
            raise self._err("glc_device_malloc")
        return p

    def dev_free(self, p):
        self.L.glc_device_free(self.h, p)

    def h2d(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        if self.L.glc_memcpy_h2d(self.h, dptr, arr.ctypes.data, arr.nbytes) != 0:
            raise self._err("glc_memcpy_h2d")

    def d2h(self, arr, dptr):
        if self.L.glc_memcpy_d2h(self.h, arr.ctypes.data, dptr, arr.nbytes) != 0:
            raise self._err("glc_memcpy_d2h")

    def forward_device(self, d_ids, d_mask, B, S, Cn, d_logits):
        if self.L.glc_engine_forward_device(self.h, d_ids, d_mask, B, S, Cn, d_logits) != 0:
            raise self._err("glc_engine_forward_device")

    def sync(self):
        if self.L.glc_engine_sync(self.h) != 0:
            raise self._err("glc_engine_sync")

    def timer_start(self):
        self.L.glc_timer_start(self.h)

    def timer_stop_ms(self):
        return float(self.L.glc_timer_stop_ms(self.h))

    def profile(self, on=True):
        self.L.glc_profile_enable(self.h, int(on))

    def profile_read(self):
        n = 16
        names = (C.c_char_p * n)()
        ms = (C.c_float * n)()
        cnt = (C.c_int * n)()
        k = self.L.glc_profile_read(self.h, names, ms, cnt, n)
        return {names[i].decode(): (float(ms[i]), int(cnt[i])) for i in range(k)}
