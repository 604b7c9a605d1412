"""GPU (-m gpu): the Qwen3 and Llama variants of the decoder backbone — per-head RMSNorm on Q and K before RoPE (qk_norm), no q / k / v
biases (attn_bias = 0), head_dim that is not hidden / heads — against the transformers fixtures of tests/golden/qwen3 and the CPU
restatement tests/decoder_ref.py (pinned on those fixtures and on live models by tests/test_qwen3_host.py).

Tolerances are the decoder and ModernBERT suites' own: probabilities 1e-4 (f32) / 1e-2 (f16) / 6e-2 (bf16), f32 hidden samples 3e-4,
f32 forwards that ran the MX pipeline 3e-4 on probabilities."""
import dataclasses
import glob
import os

import numpy as np
import pytest
import torch

import decoder_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q3_GOLDEN = os.path.join(ROOT, "tests", "golden", "qwen3")
TOL_PROB = {"f32": 1e-4, "f16": 1e-2, "bf16": 6e-2}
TOL_HIDDEN_F32 = 3e-4
TOL_PROB_MX = 3e-4


def sig(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def _fixtures(prefix):
    return sorted(glob.glob(os.path.join(Q3_GOLDEN, prefix + "*.npz")))


def _check_fixture(path, dtype, weights_for):
    from gliclass.c_amd.engine import Engine
    z = np.load(path)
    cfg, w = weights_for(str(z["config"]))
    ids, mask = z["ids"].astype(np.int64), z["mask"].astype(np.int64)
    B, S = ids.shape
    eng = Engine(cfg, w, dtype=dtype)
    try:
        eng.keep_hidden(dtype == "f32")
        got = eng.forward(ids, mask)
        assert got.shape == z["logits"].shape and np.isfinite(got).all()
        err = float(np.abs(sig(got) - z["probs"].astype(np.float64)).max())
        print(os.path.basename(path), dtype, "probability error", err)
        assert err <= TOL_PROB[dtype]
        if dtype == "f32":
            pos = z["sample_pos"]
            att = mask[:, pos].astype(bool)
            n = z["hidden_samples"].shape[-1]
            for which in range(cfg.layers + 1):
                e_h = float(np.abs(eng.hidden(which, B, S)[:, pos, :n] - z["hidden_samples"][which])[att].max())
                print("  hidden", which, e_h)
                assert e_h <= TOL_HIDDEN_F32, which
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("path", _fixtures("q3_"), ids=lambda p: os.path.basename(p)[:-4])
def test_qwen3_fixtures(path, dtype, weights_for):
    """transformers' Qwen3Model on the repo's synthetic weights: probabilities, and in f32 the hidden samples of every layer."""
    _check_fixture(path, dtype, weights_for)


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("path", _fixtures("ll_"), ids=lambda p: os.path.basename(p)[:-4])
def test_llama_fixtures(path, dtype, weights_for):
    """transformers' LlamaModel: the decoder stack without biases and without the QK norm."""
    _check_fixture(path, dtype, weights_for)


_SWEEP = ((1, 0, 21), (33, 2, 22), (129, 3, 23), (515, 4, 24))      # (S, labels, seed), B = 1
_SWEEP_REFS = {}


def _sweep_refs(cname, causal, weights_for):
    """decoder_ref (float64) on the sweep shapes, computed once per (config, mask) and shared by the three operand types."""
    from gliclass.c_amd import synth
    if (cname, causal) not in _SWEEP_REFS:
        base, w = weights_for(cname)
        cfg = dataclasses.replace(base, causal=causal)
        out = []
        for (S, Cn, seed) in _SWEEP:
            ids, mask, _ = synth.make_inputs(cfg, 1, S, Cn, seed=seed)
            out.append((ids, mask, decoder_ref.forward(cfg, w, ids, mask, dtype=torch.float64)))
        _SWEEP_REFS[(cname, causal)] = (cfg, w, out)
    return _SWEEP_REFS[(cname, causal)]


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("causal", [1, 0])
@pytest.mark.parametrize("cname", ["q3-tiny", "q3-mini"])
def test_qwen3_sweep_against_reference(cname, causal, dtype, weights_for):
    """B = 1, S in {1, 33, 129, 515} with 0 / 2 / 3 / 4 labels: the layout pass at head_dim 64 (q3-tiny) and 128 (q3-mini), as split-f16
    units (f32) and 16-bit fragments; q3-mini in f32 also with the group-split pipeline forced on and off and on the MX pipeline
    (plain projection with the permuted columns put back + the MX layout pass, which carries the norm)."""
    from gliclass.c_amd.engine import Engine
    cfg, w, refs = _sweep_refs(cname, causal, weights_for)
    eng = Engine(cfg, w, dtype=dtype)
    try:
        for (ids, mask, ref) in refs:
            S = ids.shape[1]
            got = eng.forward(ids, mask)
            assert got.shape == ref.shape and np.isfinite(got).all()
            err = float(np.abs(sig(got) - sig(ref)).max()) if ref.size else 0.0
            print(cname, causal, dtype, S, "error", err)
            assert err <= TOL_PROB[dtype], S
            if dtype != "f32" or cname != "q3-mini" or not ref.size:
                continue
            eng.set_group_split(0)
            plain = eng.forward(ids, mask)
            assert not eng.last_group_split() and not eng.last_mx()
            eng.set_group_split(2)
            eng.set_mx(False)
            gs = eng.forward(ids, mask)
            assert eng.last_group_split() and not eng.last_mx(), "the group-split pipeline did not run"
            eng.set_mx(True)
            mx = eng.forward(ids, mask)
            assert eng.last_mx() and eng.last_mx_attention(), "the MX pipeline did not run"
            assert not eng.last_rope_epilogue(), "the RoPE epilogue has no QK norm: it must not run for Qwen3"
            eng.set_group_split(1)
            e_p, e_g, e_m = (float(np.abs(sig(v) - sig(ref)).max()) for v in (plain, gs, mx))
            print("   plain", e_p, "group split", e_g, "MX", e_m)
            assert e_p <= TOL_PROB["f32"] and e_g <= TOL_PROB["f32"], S
            assert e_m <= TOL_PROB_MX, S
    finally:
        eng.close()


def test_qwen3_three_passes_agree(weights_for):
    """The in-place RoPE pass of the straightforward attention (attn_impl 1), the layout pass of the MFMA attention (default) and the
    reference agree pairwise on a ragged batch: each carries its own copy of the norm."""
    from gliclass.c_amd import synth
    from gliclass.c_amd.engine import Engine
    cfg, w = weights_for("q3-mini")
    B, S = 3, 100
    ids, mask, _ = synth.make_inputs(cfg, B, S, 3, seed=31, ragged=True, labels_per_row=[3, 1, 2])
    assert mask.sum(1).min() < S
    ref, ref_h = decoder_ref.forward(cfg, w, ids, mask, dtype=torch.float64, want_hidden=True)
    eng = Engine(cfg, w, dtype="f32")
    try:
        eng.keep_hidden(True)
        outs = {}
        for name, impl in (("rope_qk", 1), ("layout", 0)):
            eng.set_attention_impl(impl)
            logits = eng.forward(ids, mask)
            outs[name] = (logits, np.stack([eng.hidden(i, B, S) for i in range(cfg.layers + 1)]))
        eng.set_attention_impl(0)
        outs["reference"] = (ref, ref_h)
        att = mask.astype(bool)
        names = list(outs)
        for i in range(3):
            for j in range(i + 1, 3):
                (la, ha), (lb, hb) = outs[names[i]], outs[names[j]]
                e_p, e_h = float(np.abs(sig(la) - sig(lb)).max()), float(np.abs(ha - hb)[:, att].max())
                print(names[i], "vs", names[j], "probabilities", e_p, "hidden", e_h)
                assert e_p <= TOL_PROB["f32"] and e_h <= TOL_HIDDEN_F32, (names[i], names[j])
    finally:
        eng.close()


def test_qwen3_gains_are_applied_per_head_and_not_mixed_up(weights_for):
    """The same model with the gains of q and k exchanged, in the engine and in the reference: both runs match their reference and differ
    from each other by more than the bound — a q / k mix-up, or a shuffle that mixes neighbouring heads or rows, would not."""
    from gliclass.c_amd import synth
    from gliclass.c_amd.engine import Engine
    cfg, w = weights_for("q3-mini")
    B, S = 2, 64
    ids, mask, _ = synth.make_inputs(cfg, B, S, 3, seed=41, ragged=True)
    sw = dict(w)
    for l in range(cfg.layers):
        q, k = f"layers.{l}.self_attn.q_norm.weight", f"layers.{l}.self_attn.k_norm.weight"
        sw[q], sw[k] = w[k], w[q]
    att = mask.astype(bool)
    got = []
    for tensors in (w, sw):
        ref, ref_h = decoder_ref.forward(cfg, tensors, ids, mask, dtype=torch.float64, want_hidden=True)
        eng = Engine(cfg, tensors, dtype="f32")
        try:
            eng.keep_hidden(True)
            logits = eng.forward(ids, mask)
            hid = np.stack([eng.hidden(i, B, S) for i in range(cfg.layers + 1)])
        finally:
            eng.close()
        e_p, e_h = float(np.abs(sig(logits) - sig(ref)).max()), float(np.abs(hid - ref_h)[:, att].max())
        print("probabilities", e_p, "hidden", e_h)
        assert e_p <= TOL_PROB["f32"] and e_h <= TOL_HIDDEN_F32
        got.append((logits, hid))
    d_p, d_h = float(np.abs(sig(got[0][0]) - sig(got[1][0])).max()), float(np.abs(got[0][1] - got[1][1])[:, att].max())
    print("exchanged vs not: probabilities", d_p, "hidden", d_h)
    assert d_p > TOL_PROB["f32"] and d_h > TOL_HIDDEN_F32


@pytest.mark.parametrize("variant", ["ll-tiny", "even-heads"])
def test_llama_on_the_mx_pipeline(variant, weights_for):
    """A bias-free model on the forced MX pipeline.  ll-tiny has one kv head: the separate layout pass.  With even head counts the QKV
    projection takes the RoPE epilogue (EPI_QKVR), which used to hang on the permuted bias's existence."""
    from gliclass.c_amd import synth, weights
    from gliclass.c_amd.engine import Engine
    cfg, w = weights_for("ll-tiny")
    if variant == "even-heads":
        cfg = dataclasses.replace(cfg, heads=4, kv_heads=2)
        w = weights.make_weights(cfg, 13)
    ids, mask, _ = synth.make_inputs(cfg, 3, 100, 3, seed=51, ragged=True, labels_per_row=[3, 0, 2])
    ref = decoder_ref.forward(cfg, w, ids, mask, dtype=torch.float64)
    eng = Engine(cfg, w, dtype="f32")
    try:
        eng.set_group_split(2)
        got = eng.forward(ids, mask)
        assert eng.last_group_split() and eng.last_mx() and eng.last_mx_attention(), "the MX pipeline did not run"
        assert eng.last_rope_epilogue() == (variant == "even-heads")
        err = float(np.abs(sig(got) - sig(ref)).max())
        print(variant, "MX probability error", err)
        assert np.isfinite(got).all() and err <= TOL_PROB_MX
    finally:
        eng.close()


def test_qk_norm_is_refused_off_the_decoder_backbone(weights_for):
    from gliclass.c_amd import _lib
    from gliclass.c_amd.engine import Engine, to_c_config
    cfg, w = weights_for("tiny")
    cc = to_c_config(cfg)
    cc.qk_norm = 1
    import ctypes as C
    from gliclass.c_amd.weights import tensor_specs
    arrs = [np.ascontiguousarray(w[s[0]], np.float32) for s in tensor_specs(cfg)]
    ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    L = _lib.hip()
    assert not L.glc_engine_create(C.byref(cc), ptrs, len(arrs), 0, 0)
    assert b"qk_norm" in L.glc_last_error()
    assert Engine is not None


def test_qwen3_full_size_once(c_generated_weights):
    """qwen3-0.6b (28 layers, hidden 1024, 16 query / 8 kv heads of 128, SwiGLU 3072) at B = 2, S = 512 in f32 on C-generated weights,
    against the reference on the first row."""
    from gliclass.c_amd import synth
    from gliclass.c_amd.config import CONFIGS
    from gliclass.c_amd.engine import Engine
    cfg = CONFIGS["qwen3-0.6b"]
    spec = "synthetic:qwen3-0.6b:42"
    ids, mask, _ = synth.make_inputs(cfg, 2, 512, 4, seed=61, ragged=True, labels_per_row=[4, 2])
    eng = Engine.from_spec(cfg, spec, dtype="f32")
    try:
        got = eng.forward(ids, mask)
        mx = eng.last_mx()
    finally:
        eng.close()
    assert np.isfinite(got).all()
    w = c_generated_weights(spec, cfg)
    ref = decoder_ref.forward(cfg, w, ids[:1], mask[:1], dtype=torch.float64)
    err = float(np.abs(sig(got[0]) - sig(ref[0])).max())
    print("qwen3-0.6b: MX pipeline", mx, "probability error of row 0", err)
    assert err <= (TOL_PROB_MX if mx else TOL_PROB["f32"])
