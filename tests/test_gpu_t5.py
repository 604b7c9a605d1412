"""GPU (-m gpu): the T5 / mT5 backbone — the HF fixtures (tests/golden/t5) through the engine, a shape sweep on t5-tiny / t5-odd /
t5-mini against the float64 restatement tests/t5_ref.py (pinned on those fixtures by tests/test_t5_host.py), one long row, the path
checks (attention implementations, group split, last-layer pruning, length bucketing, graph replay, profiler classes), the MX
refusals and the bias-sensitivity guard.  The bars are the ones tests/test_gpu_bert.py holds the same kernels to."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

import t5_ref

pytestmark = pytest.mark.gpu

TOL_PROB = {"f32": 1e-4, "f16": 1e-2, "bf16": 6e-2}          # tests/test_gpu_bert.py TOL_PROB
TOL_HIDDEN = 3e-4                                            # ... and its f32 hidden-state bar
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("tiny_s1", "tiny_s33", "tiny_s130", "odd_rpad", "odd_lpad")


def sig(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


_ENGINES = {}
_REFS = {}


@pytest.fixture(scope="module")
def engine_for(weights_for):
    """(config name, dtype) -> one engine per module (closed at its end)"""
    from gliclass.c_amd.engine import Engine

    def get(cname, dtype):
        if (cname, dtype) not in _ENGINES:
            cfg, w = weights_for(cname)
            _ENGINES[(cname, dtype)] = Engine(cfg, w, dtype=dtype)
        return _ENGINES[(cname, dtype)]
    yield get
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


def _pad(cfg, ids, mask):
    ids = ids.copy()
    ids[mask == 0] = cfg.pad_id
    return ids


def _inputs(cfg, name):
    """the sweep's batches: (ids, mask)"""
    from gliclass.c_amd import synth
    lab, sep = cfg.class_token_index, cfg.sep_id
    if name == "b1_s1":                       # one token: the class token is the pooled row too
        return np.array([[lab]], np.int64), np.ones((1, 1), np.int64)
    if name.startswith("b2_s130_c"):          # 0 / 2 / 5 labels
        ids, mask, _ = synth.make_inputs(cfg, 2, 130, int(name[9:]), seed=130, ragged=True)
        return _pad(cfg, ids, mask), mask
    if name == "ragged_two_tokens":           # ragged masks; the last row is all pad but for two tokens
        ids, mask, _ = synth.make_inputs(cfg, 3, 100, 3, seed=8, ragged=True)
        ids[2], mask[2] = cfg.pad_id, 0
        ids[2, :2], mask[2, :2] = (lab, sep), 1
        return _pad(cfg, ids, mask), mask
    if name == "left_padded":                 # row 1 starts with 9 pad tokens, row 2 has pads inside
        ids, mask, _ = synth.make_inputs(cfg, 3, 70, 2, seed=9, ragged=False)
        ids[1, 9:], mask[1, 9:] = ids[1, :-9].copy(), 1
        ids[1, :9], mask[1, :9] = cfg.pad_id, 0
        ids[2, 20:27], mask[2, 20:27] = cfg.pad_id, 0
        ids[2, 60:], mask[2, 60:] = cfg.pad_id, 0
        return ids, mask
    B, S = {"b3_s33": (3, 33), "b3_s64": (3, 64), "b3_s65": (3, 65), "b1_s1100": (1, 1100)}[name]
    ids, mask, _ = synth.make_inputs(cfg, B, S, 2, seed=S, ragged=True)
    return _pad(cfg, ids, mask), mask


SWEEP = ["b1_s1", "b3_s33", "b3_s64", "b3_s65", "b2_s130_c0", "b2_s130_c2", "b2_s130_c5", "ragged_two_tokens", "left_padded"]


def _ref(cfg, w, cname, name):
    if (cname, name) not in _REFS:
        ids, mask = _inputs(cfg, name)
        _REFS[(cname, name)] = t5_ref.forward(cfg, w, ids, mask, want_hidden=True)
    return _REFS[(cname, name)]


def _check(eng, cfg, w, cname, name, dtype):
    ids, mask = _inputs(cfg, name)
    ref, hs = _ref(cfg, w, cname, name)
    B, S = ids.shape
    f32 = dtype == "f32"
    modes = (2, 0) if (f32 and cname == "t5-mini") else (1,)
    worst = 0.0
    outs = []
    for mode in modes:
        eng.set_group_split(mode)
        for impl in ((0, 1) if f32 else (0,)):
            eng.set_attention_impl(impl)
            got = eng.forward(ids, mask, c_alloc=ref.shape[1])
            assert got.shape == ref.shape and np.isfinite(got).all()
            if ref.size:
                err = float(np.abs(sig(got) - sig(ref)).max())
                worst = max(worst, err)
                print(f"{cname} {name} {dtype} gs {mode} impl {impl}: |prob - ref| = {err:.2e}")
                assert err <= TOL_PROB[dtype], (cname, name, dtype, mode, impl, err)
            outs.append(got)
            assert eng.last_group_split() == (mode == 2 and impl == 0), (cname, name, mode, impl)
            assert eng.last_mx() == 0 and eng.last_mx_attention() == 0
            assert eng.last_pruned() == 1            # on by default, 'first' pooling
    eng.set_attention_impl(0)
    eng.set_group_split(1)
    for o in outs[1:]:                        # attention impl 1 against the MFMA kernel, the group-split pipeline against the plain one
        if o.size:
            assert np.abs(sig(o) - sig(outs[0])).max() <= TOL_PROB[dtype]
    if f32:                                   # hidden states at attended positions (keep_hidden: plain rows, every row)
        eng.keep_hidden(True)
        try:
            eng.forward(ids, mask, c_alloc=ref.shape[1])
            assert eng.last_pruned() == 0
            att = mask.astype(bool)
            for which in range(cfg.layers + 1):
                e_h = float(np.abs(eng.hidden(which, B, S) - hs[which])[att].max())
                print(f"{cname} {name} hidden {which}: {e_h:.2e}")
                assert e_h <= TOL_HIDDEN, (cname, name, which, e_h)
        finally:
            eng.keep_hidden(False)


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("name", SWEEP)
@pytest.mark.parametrize("cname", ["t5-tiny", "t5-odd", "t5-mini"])
def test_sweep_against_reference(cname, name, dtype, weights_for, engine_for):
    cfg, w = weights_for(cname)
    _check(engine_for(cname, dtype), cfg, w, cname, name, dtype)


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_one_long_row(dtype, weights_for, engine_for):
    """t5-tiny at B = 1, S = 1100: 35 key tiles, most distances in the saturated buckets, Sp = 1152 != S"""
    cfg, w = weights_for("t5-tiny")
    _check(engine_for("t5-tiny", dtype), cfg, w, "t5-tiny", "b1_s1100", dtype)


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("case", CASES)
def test_fixtures(case, dtype):
    """The HF-initialised fixture models (+ a synthetic head) through the engine, against the restatement the fixtures pin."""
    from gliclass.c_amd.engine import Engine
    z = np.load(os.path.join(GOLDEN, "t5", case + ".npz"))
    cfg, t = t5_ref.fixture_model(GOLDEN, str(z["flavour"]))
    ids, mask = z["ids"].astype(np.int64), z["mask"].astype(np.int64)
    B, S = ids.shape
    ref, hs = t5_ref.forward(cfg, t, ids, mask, want_hidden=True)
    assert ref.size
    eng = Engine(cfg, t, dtype=dtype)
    try:
        if dtype == "f32":
            eng.keep_hidden(True)
        got = eng.forward(ids, mask)
        assert got.shape == ref.shape and np.isfinite(got).all()
        err = float(np.abs(sig(got) - sig(ref)).max())
        print(f"{case} {dtype}: |prob - ref| = {err:.2e}")
        assert err <= TOL_PROB[dtype]
        assert eng.last_mx() == 0
        if dtype == "f32":
            att = mask.astype(bool)
            for which in range(cfg.layers + 1):
                e_h = float(np.abs(eng.hidden(which, B, S) - hs[which])[att].max())
                print(f"{case} hidden {which}: {e_h:.2e}")
                assert e_h <= TOL_HIDDEN, which
            pos = z["sample_pos"]
            assert np.abs(eng.hidden(cfg.layers, B, S)[:, pos] - z["lhs_samples"])[mask[:, pos].astype(bool)].max() <= TOL_HIDDEN      # ... and HF's own numbers
    finally:
        eng.close()


def test_bias_sensitivity(weights_for):
    """An engine whose rel_bias is zeroed misses the reference by more than the f32 bar on the S = 130 case: a silently skipped bias
    cannot pass the sweep."""
    from gliclass.c_amd.engine import Engine
    cfg, w = weights_for("t5-tiny")
    ids, mask = _inputs(cfg, "b2_s130_c2")
    ref, _ = _ref(cfg, w, "t5-tiny", "b2_s130_c2")
    w0 = dict(w)
    n = "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"
    w0[n] = np.zeros_like(w[n])
    for impl in (0, 1):
        eng = Engine(cfg, w0, dtype="f32")
        try:
            eng.set_attention_impl(impl)
            got = eng.forward(ids, mask)
            err = float(np.abs(sig(got) - sig(ref)).max())
            print(f"zeroed bias, impl {impl}: |prob - ref| = {err:.2e}")
            assert err > TOL_PROB["f32"]
            assert np.abs(sig(got) - sig(t5_ref.forward(cfg, w0, ids, mask))).max() <= TOL_PROB["f32"]
        finally:
            eng.close()


@pytest.mark.parametrize("cname,name", [("t5-tiny", "b3_s65"), ("t5-odd", "left_padded"), ("t5-mini", "b2_s130_c5")])
def test_pruning_exact(cname, name, weights_for, engine_for):
    cfg, w = weights_for(cname)
    ids, mask = _inputs(cfg, name)
    eng = engine_for(cname, "f32")
    try:
        a = eng.forward(ids, mask)
        assert eng.last_pruned() == 1
        eng.set_prune_last_layer(False)
        b = eng.forward(ids, mask)
        assert eng.last_pruned() == 0
        assert np.abs(sig(a) - sig(b)).max() <= TOL_PROB["f32"]
    finally:
        eng.set_prune_last_layer(True)


def test_never_pruned_with_average_pooling(weights_for):
    from gliclass.c_amd.config import POOL_AVG
    from gliclass.c_amd.engine import Engine
    base, w = weights_for("t5-tiny")
    cfg = dataclasses.replace(base, pooling=POOL_AVG)
    ids, mask = _inputs(cfg, "b3_s33")
    eng = Engine(cfg, w, dtype="f32")
    try:
        got = eng.forward(ids, mask)
        assert eng.last_pruned() == 0
        assert np.abs(sig(got) - sig(t5_ref.forward(cfg, w, ids, mask))).max() <= TOL_PROB["f32"]
    finally:
        eng.close()


def test_length_bucketing_rows_identical(weights_for, engine_for):
    from gliclass.c_amd import synth
    cfg, w = weights_for("t5-mini")
    ids, mask, _ = synth.make_inputs(cfg, 96, 2048, 3, seed=31)
    for b in range(32, 96):                  # 32 rows of 2048 tokens, 64 of 132 - 195: the planner splits the batch (3 waves of tiles -> 2)
        mask[b, 100 + b:] = 0
    ids = _pad(cfg, ids, mask)
    eng = engine_for("t5-mini", "f32")
    eng.set_group_split(2)                   # one pipeline for every group, whatever its fill: the comparison is about the bucketing alone
    try:
        eng.set_length_buckets(4)
        a = eng.forward(ids, mask)
        groups = eng.L.glc_debug_last_forward_groups(eng.h)
        eng.set_length_buckets(1)
        b = eng.forward(ids, mask)
        assert groups > 1
        err = float(np.abs(sig(a) - sig(b)).max())
        print(f"bucketed against unbucketed rows: {err:.2e}")
        assert err <= 1e-5
    finally:
        eng.set_length_buckets(4)
        eng.set_group_split(1)


@pytest.mark.parametrize("cname,dtype", [("t5-tiny", "f32"), ("t5-mini", "f32"), ("t5-odd", "bf16")])
def test_graph_replay_bit_identical(cname, dtype, weights_for, engine_for):
    cfg, w = weights_for(cname)
    ids, mask = _inputs(cfg, "left_padded")
    eng = engine_for(cname, dtype)
    if cname == "t5-mini":
        eng.set_group_split(2)
    try:
        eager = eng.forward(ids, mask)
        eng.set_graph_replay(True)
        states = []
        for _ in range(3):
            got = eng.forward(ids, mask)
            states.append(eng.last_graph())
            assert np.array_equal(got, eager)
        assert states == [0, 1, 2]
        assert eng.last_group_split() == (cname == "t5-mini")
    finally:
        eng.set_graph_replay(False)
        eng.set_group_split(1)


def test_profiler_classes(weights_for, engine_for):
    cfg, w = weights_for("t5-tiny")
    ids, mask = _inputs(cfg, "b3_s65")
    eng = engine_for("t5-tiny", "f16")
    eng.profile(True)
    eng.set_prune_last_layer(False)
    try:
        eng.forward(ids, mask)
        full = eng.profile_read()
        eng.profile(False)
        eng.profile(True)                    # (the counts run on until the profiler is switched on again)
        eng.set_prune_last_layer(True)
        eng.forward(ids, mask)
        pruned = eng.profile_read()
    finally:
        eng.profile(False)
        eng.set_prune_last_layer(True)
    L = cfg.layers
    assert full["embed_ln"][1] == 1 and full["gemm_qkv"][1] == L and full["attention"][1] == L and full["layernorm"][1] == 2 * L + 1
    assert full["gemm_ffn1_gelu"][1] == L and full["gemm_ffn2"][1] == L and full["last_layer_pruned"][1] == 0
    assert pruned["gemm_qkv"][1] == L - 1 and pruned["attention"][1] == L - 1 and pruned["gemm_ffn2"][1] == L - 1
    assert pruned["layernorm"][1] == 2 * (L - 1) and pruned["last_layer_pruned"][1] > 0


def test_refusals(weights_for, engine_for):
    from gliclass.c_amd import _lib
    from gliclass.c_amd.engine import to_c_config
    cfg, w = weights_for("t5-mini")
    eng = engine_for("t5-mini", "f32")
    with pytest.raises(RuntimeError, match="the T5 backbone has no MX pipeline"):
        eng.enable_mx()
    with pytest.raises(RuntimeError, match="not available to this engine"):
        eng.set_mx(True)
    with pytest.raises(RuntimeError, match="t5 backbone"):
        eng.set_mx_small_forwards(1)
    eng.set_mx_small_forwards(0)                                   # off is accepted everywhere
    ok, _ = _inputs(cfg, "b3_s33")
    assert np.isfinite(eng.forward(ok, np.ones_like(ok))).all() and eng.last_mx() == 0      # ... and the engine is as it was
    # qk_norm exists on the decoder backbone only
    L = _lib.hip()
    cc = to_c_config(cfg)
    cc.qk_norm = 1
    from gliclass.c_amd.weights import tensor_specs
    arrs = [np.ascontiguousarray(w[n], np.float32) for n, _, _, _ in tensor_specs(cfg)]
    ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    assert not L.glc_engine_create(C.byref(cc), ptrs, len(arrs), 0, 0)
    assert b"qk_norm" in L.glc_last_error()


def test_synthetic_spec_and_blob_sessions(tmp_path, weights_for):
    """synthetic:t5-odd:<seed>, a .glcw blob and an HF checkpoint directory give the same engine (the C weight source
    create_ort_session uses)."""
    pytest.importorskip("safetensors")
    from gliclass.c_amd import weights
    from gliclass.c_amd.engine import Engine
    import test_t5_host
    cfg, w = weights_for("t5-odd", 9)
    ids, mask = _inputs(cfg, "b3_s65")
    eng = Engine(cfg, w, dtype="f32")
    try:
        want = eng.forward(ids, mask)
    finally:
        eng.close()
    blob = str(tmp_path / "t5.glcw")
    weights.write_blob(blob, cfg, w)
    ckpt = test_t5_host._hf_dir(tmp_path, cfg, w, "mt5")
    for spec in ("synthetic:t5-odd:9", blob, ckpt):
        eng = Engine.from_spec(cfg, spec, dtype="f32")
        try:
            assert np.array_equal(eng.forward(ids, mask), want), spec
        finally:
            eng.close()
