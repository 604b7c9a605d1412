"""GPU (-m gpu): the BERT / RoBERTa / XLM-R backbone — the HF fixtures (tests/golden/bert) through the engine, a shape sweep on
bert-tiny / bert-mini against the float64 restatement tests/bert_ref.py (pinned on those fixtures by tests/test_bert_host.py), the
position ids bit for bit, length bucketing, graph replay, and everything the backbone refuses.  Tolerances are the ModernBERT suite's
for the same kernels (fp32 is the parity-grade mode; the 16-bit modes are held to their measured envelope)."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

import bert_ref

pytestmark = pytest.mark.gpu

TOL_PROB = {"f32": 1e-4, "f16": 1e-2, "bf16": 6e-2}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("bert_s1", "bert_s33", "bert_s130", "roberta_rpad", "roberta_lpad")


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
    lab, sep, cls = cfg.class_token_index, cfg.sep_id, cfg.cls_id
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
    if name == "left_padded":                 # RoBERTa-style: row 1 starts with 9 pad tokens, row 2 has pads inside
        ids, mask, _ = synth.make_inputs(cfg, 3, 70, 2, seed=9, ragged=False)
        ids[1, 9:], mask[1, 9:] = ids[1, :-9].copy(), 1
        ids[1, :9], mask[1, :9] = cfg.pad_id, 0
        ids[2, 20:27], mask[2, 20:27] = cfg.pad_id, 0
        ids[2, 60:], mask[2, 60:] = cfg.pad_id, 0
        return ids, mask
    if name == "table_end":                   # S = max_positions - pos_offset: the last row of the table is read
        S = cfg.max_positions - cfg.pos_offset
        ids, mask, _ = synth.make_inputs(cfg, 1, S, 2, seed=3, ragged=False)
        return ids, mask
    B, S = {"b3_s33": (3, 33), "b3_s64": (3, 64), "b3_s65": (3, 65), "b2_s1500": (2, 1500)}[name]
    ids, mask, _ = synth.make_inputs(cfg, B, S, 2, seed=S, ragged=True)
    return _pad(cfg, ids, mask), mask


SWEEP = ["b1_s1", "b3_s33", "b3_s64", "b3_s65", "b2_s130_c0", "b2_s130_c2", "b2_s130_c5", "ragged_two_tokens", "left_padded", "table_end"]


def _check(eng, cfg, w, cname, name, dtype):
    ids, mask = _inputs(cfg, name)
    if (cname, name) not in _REFS:
        _REFS[(cname, name)] = bert_ref.forward(cfg, w, ids, mask)
    ref = _REFS[(cname, name)]
    B, S = ids.shape
    f32 = dtype == "f32"
    modes = (2, 0) if (f32 and cname == "bert-mini") else (1,)
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
                assert err <= TOL_PROB[dtype], (cname, name, dtype, mode, impl, err)
            outs.append(got)
            assert eng.last_group_split() == (mode == 2 and impl == 0), (cname, name, mode, impl)
            assert eng.last_mx() == 0 and eng.last_mx_attention() == 0 and eng.last_pruned() == 0
    eng.set_attention_impl(0)
    eng.set_group_split(1)
    for o in outs[1:]:                        # the attention kernels (and the two pipelines) agree with each other
        if o.size:
            assert np.abs(sig(o) - sig(outs[0])).max() <= TOL_PROB[dtype]
    print(f"{cname} {name} {dtype}: worst |prob - ref| = {worst:.2e}")
    # the position ids as the embedding kernel read them: bit-exact, slack positions on a row that exists
    pos = eng.pos_ids(B, S)
    assert np.array_equal(pos[:, :S], bert_ref.position_ids(cfg, ids))
    assert (pos[:, S:] == (cfg.pad_id if cfg.pos_offset else 0)).all() and pos.max() < cfg.max_positions


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("name", SWEEP)
@pytest.mark.parametrize("cname", ["bert-tiny", "bert-mini"])
def test_sweep_against_reference(cname, name, dtype, weights_for, engine_for):
    cfg, w = weights_for(cname)
    _check(engine_for(cname, dtype), cfg, w, cname, name, dtype)


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_long_rows(dtype, weights_for, engine_for):
    """bert-mini at B = 2, S = 1500: every thread of the position scan holds several ids, the counts cross the waves of the workgroup"""
    cfg, w = weights_for("bert-mini")
    _check(engine_for("bert-mini", dtype), cfg, w, "bert-mini", "b2_s1500", dtype)


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("case", CASES)
def test_fixtures(case, dtype):
    """The HF-initialised fixture models (+ a synthetic head) through the engine, against the restatement the fixtures pin."""
    from gliclass.c_amd.engine import Engine
    z = np.load(os.path.join(GOLDEN, "bert", case + ".npz"))
    cfg, t = bert_ref.fixture_model(GOLDEN, str(z["flavour"]))
    ids, mask = z["ids"].astype(np.int64), z["mask"].astype(np.int64)
    B, S = ids.shape
    ref, hs = bert_ref.forward(cfg, t, ids, mask, want_hidden=True)
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
        assert eng.last_mx() == 0 and eng.last_pruned() == 0
        if dtype == "f32":
            att = mask.astype(bool)
            for which in range(cfg.layers + 1):
                e_h = float(np.abs(eng.hidden(which, B, S) - hs[which])[att].max())
                print(f"{case} hidden {which}: {e_h:.2e}")
                assert e_h <= 3e-4, which
            pos = z["sample_pos"]
            assert np.abs(eng.hidden(cfg.layers, B, S)[:, pos] - z["lhs_samples"])[mask[:, pos].astype(bool)].max() <= 3e-4      # ... and HF's own numbers
    finally:
        eng.close()


def test_position_ids_bert_flavour(weights_for):
    """pos_offset = 0 numbers the positions 0 .. S-1 whatever the ids hold; the RoBERTa flavour is checked in every case of the sweep."""
    from gliclass.c_amd import weights
    from gliclass.c_amd.engine import Engine
    base, _ = weights_for("bert-tiny")
    cfg = dataclasses.replace(base, pad_id=0, cls_id=1, pos_offset=0, max_positions=128)
    w = weights.make_weights(cfg, 3)
    ids, mask = _inputs(cfg, "left_padded")
    ref = bert_ref.forward(cfg, w, ids, mask)
    eng = Engine(cfg, w, dtype="f32")
    try:
        got = eng.forward(ids, mask)
        assert np.abs(sig(got) - sig(ref)).max() <= TOL_PROB["f32"]
        pos = eng.pos_ids(*ids.shape)
        assert np.array_equal(pos[:, :70], np.broadcast_to(np.arange(70), (3, 70))) and (pos[:, 70:] == 0).all()
    finally:
        eng.close()


def test_length_bucketing_rows_identical(weights_for, engine_for):
    from gliclass.c_amd import synth
    cfg, w = weights_for("bert-mini")
    ids, mask, _ = synth.make_inputs(cfg, 96, 2048, 3, seed=31)      # (2048 = max_positions - pos_offset)
    for b in range(32, 96):                  # 32 rows of 2048 tokens, 64 of 132 - 195: the planner splits the batch (3 waves of tiles -> 2)
        n = 100 + b
        mask[b, n:] = 0
    ids = _pad(cfg, ids, mask)
    eng = engine_for("bert-mini", "f32")
    try:
        eng.set_length_buckets(4)
        a = eng.forward(ids, mask)
        groups = eng.L.glc_debug_last_forward_groups(eng.h)
        eng.set_length_buckets(1)
        b = eng.forward(ids, mask)
        assert groups > 1
        assert np.abs(sig(a) - sig(b)).max() <= 1e-5
    finally:
        eng.set_length_buckets(4)


@pytest.mark.parametrize("cname,dtype", [("bert-tiny", "f32"), ("bert-mini", "f32"), ("bert-tiny", "bf16")])
def test_graph_replay_bit_identical(cname, dtype, weights_for, engine_for):
    cfg, w = weights_for(cname)
    ids, mask = _inputs(cfg, "left_padded")
    eng = engine_for(cname, dtype)
    if cname == "bert-mini":
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
        assert eng.last_group_split() == (cname == "bert-mini")
    finally:
        eng.set_graph_replay(False)
        eng.set_group_split(1)


def test_profiler_classes(weights_for, engine_for):
    cfg, w = weights_for("bert-tiny")
    ids, mask = _inputs(cfg, "b3_s65")
    eng = engine_for("bert-tiny", "f16")
    eng.profile(True)
    try:
        eng.forward(ids, mask)
        prof = eng.profile_read()
    finally:
        eng.profile(False)
    L = cfg.layers
    assert prof["embed_ln"][1] == 1 and prof["gemm_qkv"][1] == L and prof["attention"][1] == L and prof["layernorm"][1] == 2 * L
    assert prof["gemm_ffn1_gelu"][1] == L and prof["gemm_ffn2"][1] == L and prof["last_layer_pruned"][1] == 0


def test_refusals(weights_for, engine_for):
    from gliclass.c_amd import _lib, synth
    from gliclass.c_amd.engine import to_c_config
    cfg, w = weights_for("bert-tiny")
    eng = engine_for("bert-tiny", "f32")
    S = cfg.max_positions - cfg.pos_offset + 1                     # one token more than the position table holds: an error, not a clamp
    ids, mask, _ = synth.make_inputs(cfg, 1, S, 2, seed=3)
    with pytest.raises(RuntimeError, match="max_positions - pos_offset = 512"):
        eng.forward(ids, mask)
    d = eng.dev_alloc(8 * S)
    try:
        with pytest.raises(RuntimeError, match="max_positions - pos_offset"):
            eng.forward_device(d, d, 1, S, 1, d)
    finally:
        eng.dev_free(d)
    with pytest.raises(RuntimeError, match="the BERT backbone has no MX pipeline"):
        eng.enable_mx()
    with pytest.raises(RuntimeError):
        eng.set_mx(True)
    with pytest.raises(RuntimeError, match="bert backbone"):
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
    """synthetic:bert-tiny:<seed>, a .glcw blob and an HF checkpoint directory give the same engine (the C weight source
    create_ort_session uses)."""
    pytest.importorskip("safetensors")
    from gliclass.c_amd import weights
    from gliclass.c_amd.engine import Engine
    import test_bert_host
    cfg, w = weights_for("bert-tiny", 9)
    ids, mask = _inputs(cfg, "b3_s65")
    eng = Engine(cfg, w, dtype="f32")
    try:
        want = eng.forward(ids, mask)
    finally:
        eng.close()
    blob = str(tmp_path / "bert.glcw")
    weights.write_blob(blob, cfg, w)
    ckpt = test_bert_host._hf_dir(tmp_path, dataclasses.replace(cfg, pos_buckets=0, max_rel_pos=0), w, "xlm-roberta")
    for spec in ("synthetic:bert-tiny:9", blob, ckpt):
        eng = Engine.from_spec(cfg, spec, dtype="f32")
        try:
            assert np.array_equal(eng.forward(ids, mask), want), spec
        finally:
            eng.close()
