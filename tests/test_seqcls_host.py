"""CPU: the sequence-classification head (head_kind = 1) without a GPU — the float64 reference tests/seqcls_ref.py on the transformers fixtures of
tests/golden/seqcls, the version-7 blob (and versions 2-6 byte for byte as before), the checkpoint importer with its refusals, the C-ABI's
symbols and prototypes, and the refusals glc_engine_create makes before it looks for a device."""
import ctypes as C
import dataclasses
import importlib.util
import json
import os

import numpy as np
import pytest

import seqcls_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ("deberta", "bert", "roberta", "modernbert", "modernbert_mean")

_spec = importlib.util.spec_from_file_location("gen_seqcls_golden", os.path.join(ROOT, "scripts", "gen_seqcls_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.mark.parametrize("family", FAMILIES)
def test_reference_reproduces_the_hf_fixtures(family, golden_dir):
    """1e-5 on the logits, the bar of the backbone references: the reference runs in float64 on the float32 weights, the fixtures are
    transformers' float32 logits (generation error ~1e-6 .. 8e-6 at these sizes, printed by the generator)."""
    z = np.load(os.path.join(golden_dir, "seqcls", family + ".npz"))
    meta = json.loads(str(z["config_json"]))
    assert (meta["base"], meta["overrides"]) == (gen.FAMILIES[family][0], gen.FAMILIES[family][1])
    cfg = gen.family_config(family)
    w = gen.family_weights(family, cfg, int(z["seed"]))
    assert sorted(z["absent"]) == sorted(gen.ABSENT.get(family, ()))
    assert 2 <= len(z["case_names"]) <= 3
    for name in z["case_names"]:
        ids, mask, want = z[name + ".ids"].astype(np.int64), z[name + ".mask"].astype(np.int64), z[name + ".logits"]
        got = seqcls_ref.forward(cfg, w, ids, mask)
        assert got.shape == want.shape == (ids.shape[0], cfg.cls_labels)
        assert np.abs(got - want).max() <= 1e-5, (family, name, np.abs(got - want).max())
        # the fixture sees every stage of the head
        assert np.abs(seqcls_ref.forward(cfg, w, ids, mask, act=0) - want).max() > 1e-2
        if cfg.cls_norm:
            assert np.abs(seqcls_ref.forward(cfg, w, ids, mask, norm=0) - want).max() > 1e-2
        if "cls.dense.bias" in w:
            assert np.abs(seqcls_ref.forward(cfg, w, ids, mask, dense_bias=False) - want).max() > 1e-2


def test_nli_reference_is_the_pipelines_postprocess():
    """the restatement against the lines of ZeroShotClassificationPipeline.postprocess, run on numpy as the pipeline runs them"""
    rng = np.random.default_rng(1)
    T, Lb = 3, 4
    logits = rng.normal(0, 3, (T * Lb, 3))
    reshaped = logits.reshape((T, Lb, -1))
    for en in (0, 2):
        co = 2 - en
        ec = reshaped[..., [co, en]]
        want = (np.exp(ec) / np.exp(ec).sum(-1, keepdims=True))[..., 1]
        assert np.allclose(seqcls_ref.nli_scores(logits, T, Lb, en, co, 1), want, atol=1e-12)
        el = reshaped[..., en]
        want = np.exp(el) / np.exp(el).sum(-1, keepdims=True)
        assert np.allclose(seqcls_ref.nli_scores(logits, T, Lb, en, co, 0), want, atol=1e-12)


def _blob_bytes(tmp_path, cfg, w):
    from gliclass.c_amd import weights
    p = str(tmp_path / "m.glcw")
    weights.write_blob(p, cfg, w)
    return open(p, "rb").read()


@pytest.mark.parametrize("cname,version", [("tiny", 2), ("dec-tiny", 2), ("mb-tiny", 3), ("q3-tiny", 4), ("bert-tiny", 5), ("t5-tiny", 6)])
def test_older_blob_versions_are_byte_identical(cname, version, tmp_path):
    """One config per backbone re-serialised: the 256 header bytes equal the layout of versions 2 - 6 restated here slot by slot (the version
    each backbone always had, zeros behind its last slot: no new field leaks in), and the whole file is reproduced byte for byte from its
    own reading.  (No bytes recorded from an earlier build are compared: the layout below is the record.)"""
    import struct
    from gliclass.c_amd import weights
    from gliclass.c_amd.config import CONFIGS
    cfg = CONFIGS[cname]
    w = weights.make_weights(cfg, 1)
    raw = _blob_bytes(tmp_path, cfg, w)
    d = cfg.asdict()
    ints = ["vocab", "hidden", "layers", "heads", "head_dim", "inter", "pos_buckets", "max_rel_pos", "pad_id", "cls_id", "sep_id", "class_token_index",
            "text_token_index", "pooling", "scorer", "embed_class_token", "normalize_features", "backbone", "kv_heads", "causal"]
    want = b"GLCW\x00\x01\x00\x00" + struct.pack("<II", version, len(weights.tensor_specs(cfg))) + struct.pack("<20i", *[d[k] for k in ints])
    want += struct.pack("<3f", d["ln_eps"], d["logit_scale"], d["rope_theta"])
    if version >= 3:
        want += struct.pack("<2if", d["local_window"], d["global_every"], d["rope_theta_local"])
    if version >= 4:
        want += struct.pack("<2i", d["qk_norm"], d["attn_bias"])
    if version >= 5:
        want += struct.pack("<3i", d["max_positions"], d["type_vocab"], d["pos_offset"])
    if version >= 6:
        want += struct.pack("<2i", d["rel_buckets"], d["rel_max_distance"])
    assert raw[:256] == want + b"\x00" * (256 - len(want))
    cfg2, w2 = weights.read_blob(str(tmp_path / "m.glcw"))
    assert cfg2.head_kind == 0 and cfg2.cls_labels == 0
    (tmp_path / "again").mkdir()
    assert _blob_bytes(tmp_path / "again", dataclasses.replace(cfg2, name=cfg.name), w2) == raw


@pytest.mark.parametrize("family", FAMILIES)
def test_version_7_round_trip(family, tmp_path):
    from gliclass.c_amd import _lib, weights
    cfg = gen.family_config(family)
    w = gen.family_weights(family, cfg)
    raw = _blob_bytes(tmp_path, cfg, w)
    assert raw[8:12] == b"\x07\x00\x00\x00"
    cfg2, w2 = weights.read_blob(str(tmp_path / "m.glcw"))
    for f in ("head_kind", "cls_labels", "cls_act", "cls_norm", "cls_dense", "pooling", "backbone", "hidden", "layers", "max_positions", "pos_offset", "local_window"):
        assert getattr(cfg2, f) == getattr(cfg, f), f
    assert sorted(w2) == sorted(w) and all(np.array_equal(w2[k], w[k]) for k in w)
    # the C reader: six head slots, the absent tensors null
    M = _lib.model()
    cw = _lib.Weights()
    assert M.glc_weights_load(str(tmp_path / "m.glcw").encode(), C.byref(cw)) == 0
    try:
        assert cw.cfg.head_kind == 1 and cw.cfg.cls_labels == cfg.cls_labels and cw.cfg.cls_act == cfg.cls_act
        n = cw.n_tensors
        for k, name in enumerate(weights.CLS_HEAD_NAMES):
            assert bool(cw.tensors[n - 6 + k]) == (name in w), name
        K, H = cfg.cls_labels, cfg.hidden
        assert np.array_equal(np.ctypeslib.as_array(cw.tensors[n - 2], shape=(K, H)), w["cls.classifier.weight"])
    finally:
        M.glc_weights_free(C.byref(cw))


@pytest.mark.parametrize("family", FAMILIES)
def test_importer_reads_a_saved_checkpoint(family, tmp_path):
    """model.save_pretrained of the fixture generator's HF model -> load_seqcls_checkpoint gives back the config and the tensors it ran with"""
    pytest.importorskip("safetensors")
    from gliclass.c_amd import weights
    cfg = gen.family_config(family)
    w = gen.family_weights(family, cfg)
    model = gen.build_hf(family, cfg, w)
    model.config.architectures = [type(model).__name__]
    model.save_pretrained(str(tmp_path), safe_serialization=True)
    cfg2, w2 = weights.load_seqcls_checkpoint(str(tmp_path))
    for f in ("head_kind", "cls_labels", "cls_act", "cls_norm", "cls_dense", "pooling", "backbone", "vocab", "hidden", "layers", "heads", "inter", "pad_id",
              "max_positions", "type_vocab", "pos_offset", "local_window", "global_every") + (("pos_buckets", "max_rel_pos") if family == "deberta" else ()):
        assert getattr(cfg2, f) == getattr(cfg, f), f
    assert abs(cfg2.ln_eps - cfg.ln_eps) < 1e-12 and cfg2.rope_theta == cfg.rope_theta and cfg2.rope_theta_local == cfg.rope_theta_local
    assert sorted(w2) == sorted(w)
    for k in w:
        assert np.array_equal(np.asarray(w2[k], np.float32), w[k]), k


@pytest.mark.parametrize("family", FAMILIES)
def test_c_reader_and_python_importer_agree(family, tmp_path):
    """The saved directory through the C checkpoint reader (glc_weights_load, what create_ort_session calls) and through
    weights.load_seqcls_checkpoint: the same configuration, the same six head slots (an absent tensor a null pointer), the same numbers —
    this holds the two restatements of the field checks and of the tensor names together."""
    pytest.importorskip("safetensors")
    from gliclass.c_amd import _lib, weights
    from gliclass.c_amd.engine import to_c_config
    cfg = gen.family_config(family)
    model = gen.build_hf(family, cfg, gen.family_weights(family, cfg))
    model.config.architectures = [type(model).__name__]
    model.save_pretrained(str(tmp_path), safe_serialization=True)
    pcfg, pw = weights.load_seqcls_checkpoint(str(tmp_path))
    M = _lib.model()
    cw = _lib.Weights()
    assert M.glc_weights_load(str(tmp_path).encode(), C.byref(cw)) == 0
    try:
        want = to_c_config(pcfg)
        for f, _ in _lib.ModelConfig._fields_:
            if f in ("cls_id", "sep_id", "class_token_index", "text_token_index", "kv_heads", "causal", "rope_theta", "rope_theta_local", "global_every",
                     "local_window", "pos_buckets", "max_rel_pos", "embed_class_token"):
                continue                                  # (fields this head never reads, or that only another backbone reads: compared below where they matter)
            a, b = getattr(cw.cfg, f), getattr(want, f)
            assert (abs(a - b) <= 1e-12 * max(abs(b), 1) if isinstance(b, float) else a == b), f
        if family == "deberta":
            assert (cw.cfg.pos_buckets, cw.cfg.max_rel_pos) == (pcfg.pos_buckets, pcfg.max_rel_pos)
        if family.startswith("modernbert"):
            assert (cw.cfg.local_window, cw.cfg.global_every, cw.cfg.rope_theta, cw.cfg.rope_theta_local) == \
                   (pcfg.local_window, pcfg.global_every, pcfg.rope_theta, pcfg.rope_theta_local)
        full = dataclasses.replace(pcfg, cls_dense=1, cls_norm=1)
        specs = weights.tensor_specs(full)
        assert cw.n_tensors == len(specs)
        for i, (name, shape, _, _) in enumerate(specs):
            if name not in pw:
                assert name.startswith("cls.") and not cw.tensors[i], name
                continue
            assert np.array_equal(np.ctypeslib.as_array(cw.tensors[i], shape=tuple(shape)), np.asarray(pw[name], np.float32)), name
    finally:
        M.glc_weights_free(C.byref(cw))


def _root(family):
    cfg = gen.family_config(family)
    model = gen.build_hf(family, cfg, gen.family_weights(family, cfg))
    root = json.loads(model.config.to_json_string())
    root["architectures"] = [type(model).__name__]
    return root


@pytest.mark.parametrize("family,field,value,word", [
    ("deberta", "pooler_hidden_size", 64, "pooler_hidden_size"), ("deberta", "pooler_hidden_act", "tanh", "pooler_hidden_act"),
    ("deberta", "share_att_key", False, "share_att_key"), ("deberta", "position_biased_input", True, "position_biased_input"),
    ("bert", "position_embedding_type", "relative_key", "position_embedding_type"), ("roberta", "hidden_act", "relu", "hidden_act"),
    ("modernbert", "classifier_activation", "silu", "classifier_activation"), ("modernbert", "classifier_pooling", "max", "classifier_pooling"),
    ("modernbert", "norm_bias", True, "norm_bias"), ("bert", "model_type", "qwen2", "model_type"), ("bert", "model_type", "t5", "model_type"),
    ("bert", "architectures", ["BertModel"], "architectures"), ("roberta", "id2label", {str(i): str(i) for i in range(1025)}, "num_labels"),
])
def test_importer_refusals_name_the_field(family, field, value, word, tmp_path, capfd):
    """... in the Python importer and in the C checkpoint reader alike (the C reader refuses on config.json alone, before it opens the tensors)"""
    from gliclass.c_amd import _lib, weights
    root = _root(family)
    weights.seqcls_config_from_hf(dict(root))                     # (accepted as it is)
    root[field] = value
    with pytest.raises(ValueError, match=word):
        weights.seqcls_config_from_hf(root)
    (tmp_path / "config.json").write_text(json.dumps(root))
    cw = _lib.Weights()
    capfd.readouterr()
    assert _lib.model().glc_weights_load(str(tmp_path).encode(), C.byref(cw)) != 0
    msg = capfd.readouterr().err
    if field != "architectures":                                  # (without the class name the C reader takes it for a GLiClass directory and misses the tensors)
        assert "checkpoint config" in msg and (word in msg or field in msg), msg


def test_symbols_and_prototypes():
    from gliclass.c_amd import _lib
    L = _lib.hip()
    assert hasattr(L, "glc_engine_nli_scores") and "glc_engine_nli_scores" in _lib.HIP_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "gliclass_hip.h")).read()
    assert "int glc_engine_nli_scores(glc_engine* e, const float* d_logits, int T, int Lb, int entail_id, int contra_id, int multi_label, float* d_probs);" in hdr
    assert "int32_t head_kind, cls_labels, cls_act, cls_norm, cls_dense;" in hdr and "#define GLC_TENSORS_CLS_HEAD 6" in hdr
    krn = open(os.path.join(ROOT, "gliclass", "c_amd", "csrc", "glc_kernels.h")).read()
    assert "const char* glc_launch_cls_head(" in krn and "const char* glc_launch_nli_scores(" in krn
    assert C.sizeof(_lib.ModelConfig) == 4 * 38
    assert L.glc_engine_nli_scores(None, None, 3, 4, 0, 2, 0, None) == -1 and b"null engine" in L.glc_last_error()


@pytest.mark.parametrize("cname,word", [("dec-tiny", b"decoder"), ("q3-tiny", b"decoder"), ("t5-tiny", b"T5")])
def test_create_refuses_the_head_on_decoder_and_t5_backbones(cname, word):
    """glc_engine_create checks the configuration before it counts tensors or looks for a device: this runs without a GPU"""
    from gliclass.c_amd import _lib
    from gliclass.c_amd.config import CONFIGS
    from gliclass.c_amd.engine import to_c_config
    L = _lib.hip()
    cc = to_c_config(CONFIGS[cname])
    cc.head_kind, cc.cls_labels, cc.cls_act, cc.cls_dense = 1, 3, 1, 1
    ptrs = (C.c_void_p * 1)()
    assert not L.glc_engine_create(C.byref(cc), ptrs, 1, 0, 0)
    assert word in L.glc_last_error() and b"head_kind = 1" in L.glc_last_error()
    for field, val, msg in (("cls_labels", 0, b"cls_labels"), ("cls_labels", 1025, b"cls_labels"), ("cls_act", 3, b"cls_act"), ("head_kind", 2, b"head_kind")):
        cc = to_c_config(CONFIGS["tiny"])
        cc.head_kind, cc.cls_labels, cc.cls_act, cc.cls_dense = 1, 3, 1, 1
        setattr(cc, field, val)
        assert not L.glc_engine_create(C.byref(cc), ptrs, 1, 0, 0) and msg in L.glc_last_error()
    cc = to_c_config(CONFIGS["tiny"])
    cc.cls_labels = 3                                              # a GLiClass-head config must leave the new fields 0
    assert not L.glc_engine_create(C.byref(cc), ptrs, 1, 0, 0) and b"head_kind = 0" in L.glc_last_error()
