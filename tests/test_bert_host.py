"""BERT / RoBERTa / XLM-R backbone, host side (no GPU): the float64 restatement against the committed HF fixtures, the C config /
tensor-spec mirror, the v5 blob header, and the checkpoint importers (C and Python) with their refusals."""
import ctypes as C
import dataclasses
import glob
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import bert_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BERT_CONFIGS = ("bert-tiny", "bert-mini", "bert-base")
CASES = ("bert_s1", "bert_s33", "bert_s130", "roberta_rpad", "roberta_lpad")


@pytest.fixture(scope="module")
def libs():
    from gliclass.c_amd import _lib
    return _lib, _lib.model()


def test_fixture_set_is_complete():
    names = {os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, "bert", "*.npz"))}
    assert names == set(CASES) | {"bert_weights", "roberta_weights"}
    assert all(os.path.getsize(f) < 700 * 1024 for f in glob.glob(os.path.join(GOLDEN, "bert", "*.npz")))


@pytest.mark.parametrize("case", CASES)
def test_reference_matches_fixtures(case):
    z = np.load(os.path.join(GOLDEN, "bert", case + ".npz"))
    cfg, t = bert_ref.fixture_model(GOLDEN, str(z["flavour"]))
    ids, mask = z["ids"].astype(np.int64), z["mask"].astype(np.int64)
    hs = bert_ref.backbone(cfg, t, ids, mask)
    pos = z["sample_pos"]
    att = mask[:, pos].astype(bool)
    e_l = np.abs(hs[-1][:, pos] - z["lhs_samples"])[att].max()
    print(case, "last_hidden_state samples", e_l)
    assert e_l <= 1e-5
    if "hidden_states" in z.files:
        e_h = np.abs(np.stack(hs) - z["hidden_states"])[:, mask.astype(bool)].max()
        print(case, "hidden states", e_h)
        assert e_h <= 1e-4
    else:
        assert ids.shape[1] > 64


def test_reference_sees_the_position_ids():
    """RoBERTa numbers the non-pad tokens: arange positions give another answer on the left-padded / interior-pad rows."""
    z = np.load(os.path.join(GOLDEN, "bert", "roberta_lpad.npz"))
    cfg, t = bert_ref.fixture_model(GOLDEN, "roberta")
    ids, mask = z["ids"].astype(np.int64), z["mask"].astype(np.int64)
    p = bert_ref.position_ids(cfg, ids)
    S = ids.shape[1]
    naive = np.broadcast_to(np.arange(S) + cfg.pos_offset, ids.shape)
    assert np.array_equal(p[0], naive[0]) and not np.array_equal(p[1], naive[1]) and not np.array_equal(p[2], naive[2])
    assert (p[ids == cfg.pad_id] == cfg.pad_id).all() and p[1, 7] == cfg.pos_offset
    a, b = bert_ref.backbone(cfg, t, ids, mask)[-1], bert_ref.backbone(cfg, t, ids, mask, pos_ids=naive)[-1]
    assert np.abs(a - b)[mask.astype(bool)].max() > 1e-2
    # BERT: positions 0 .. S-1 whatever the ids
    cb, _ = bert_ref.fixture_model(GOLDEN, "bert")
    assert np.array_equal(bert_ref.position_ids(cb, ids), np.broadcast_to(np.arange(S), ids.shape))


def test_fixture_weights_are_not_defaults():
    """A dropped bias, LayerNorm bias or token-type row would be visible: none of them is 0 / 1."""
    for flavour in ("bert", "roberta"):
        _, t = bert_ref.fixture_model(GOLDEN, flavour)
        assert np.abs(t["embeddings.token_type_embeddings.weight"][0]).max() > 0.1
        for n, v in t.items():
            if "projector" in n:                     # (the synthetic head: not part of the fixture)
                continue
            if n.endswith("LayerNorm.weight"):
                assert np.abs(v - 1).max() > 0.1, n
            elif n.endswith(".bias"):
                assert np.abs(v).max() > 0.05, n


def test_named_configs_and_tensor_specs_match_python(libs):
    _lib, model = libs
    from gliclass.c_amd import weights
    from gliclass.c_amd.config import CONFIGS, BACKBONE_BERT
    for cname in BERT_CONFIGS:
        cfg = CONFIGS[cname]
        assert cfg.backbone == BACKBONE_BERT == 3 and cfg.head_dim == 64 and (cfg.qk_norm, cfg.attn_bias) == (0, 1)
        cc = _lib.ModelConfig()
        assert model.glc_named_config(cname.encode(), C.byref(cc)) == 0
        assert abs(cc.ln_eps / cfg.ln_eps - 1) < 1e-6
        for f in ("vocab", "hidden", "layers", "heads", "head_dim", "inter", "pad_id", "cls_id", "sep_id", "class_token_index", "text_token_index",
                  "backbone", "kv_heads", "causal", "pooling", "scorer", "embed_class_token", "normalize_features", "qk_norm", "attn_bias",
                  "max_positions", "type_vocab", "pos_offset"):
            assert getattr(cc, f) == getattr(cfg, f), (cname, f)
        specs = weights.tensor_specs(cfg)
        buf = C.create_string_buffer(96)
        shp = (C.c_uint64 * 4)()
        amp, mean = C.c_double(), C.c_double()
        for i, (n, shape, a, m) in enumerate(specs):
            nd = model.glc_tensor_spec(C.byref(cc), i, buf, shp, C.byref(amp), C.byref(mean))
            assert nd == len(shape) and buf.value.decode() == n and tuple(shp[:nd]) == tuple(shape), (cname, i, n)
            assert abs(amp.value - a) < 1e-15 and mean.value == m
        assert model.glc_tensor_spec(C.byref(cc), len(specs), buf, shp, C.byref(amp), C.byref(mean)) == -1
        assert len(specs) == 5 + 12 * cfg.layers + 8
    t, m, b = (CONFIGS[n] for n in BERT_CONFIGS)
    assert (t.hidden, t.heads, t.layers, t.inter, t.max_positions, t.type_vocab, t.pos_offset, t.pad_id) == (128, 2, 3, 512, 514, 2, 2, 1)
    assert (m.hidden, m.heads, m.layers, m.inter, m.max_positions, m.type_vocab, m.pos_offset) == (256, 4, 4, 1024, 2050, 1, 2)
    assert (b.hidden, b.heads, b.layers, b.inter, b.vocab, b.max_positions, b.type_vocab, b.pos_offset) == (768, 12, 12, 3072, 30522, 512, 2, 0)


def test_synthetic_weights_bit_identical_to_python(libs, c_generated_weights):
    from gliclass.c_amd import weights
    from gliclass.c_amd.config import CONFIGS
    cfg = CONFIGS["bert-tiny"]
    ref = weights.make_weights(cfg, 9)
    got = c_generated_weights("synthetic:bert-tiny:9", cfg)
    assert list(got) == list(ref) and all(np.array_equal(got[k], ref[k]) for k in ref)


def test_blob_v5_round_trip_and_older_headers_unchanged(libs, tmp_path):
    _lib, model = libs
    from gliclass.c_amd import weights
    from gliclass.c_amd.config import CONFIGS
    cfg = dataclasses.replace(CONFIGS["bert-tiny"], max_positions=77, type_vocab=3, layers=2)
    ref = weights.make_weights(cfg, 7)
    path = str(tmp_path / "bert.glcw")
    weights.write_blob(path, cfg, ref)
    with open(path, "rb") as f:
        hdr = f.read(256)
    assert struct.unpack_from("<I", hdr, 8)[0] == 5
    assert struct.unpack_from("<3i", hdr, 16 + 4 * 28) == (77, 3, 2) and hdr[16 + 4 * 31:] == b"\x00" * (256 - 16 - 4 * 31)
    cfg2, back = weights.read_blob(path)
    assert dataclasses.replace(cfg2, name=cfg.name, ln_eps=cfg.ln_eps) == cfg and abs(cfg2.ln_eps / cfg.ln_eps - 1) < 1e-6
    assert all(np.array_equal(back[n], ref[n]) for n in ref)
    W = _lib.Weights()
    assert model.glc_weights_load(path.encode(), C.byref(W)) == 0
    try:
        assert (W.cfg.backbone, W.cfg.max_positions, W.cfg.type_vocab, W.cfg.pos_offset, W.cfg.pad_id) == (3, 77, 3, 2, 1)
        assert W.n_tensors == len(ref)
        for i, (n, shape, _, _) in enumerate(weights.tensor_specs(cfg)):
            assert np.array_equal(np.ctypeslib.as_array(W.tensors[i], shape=shape), ref[n])
    finally:
        model.glc_weights_free(C.byref(W))
    # a v5 header on another backbone (or a BERT blob under an older version) is refused
    raw = bytearray(open(path, "rb").read())
    struct.pack_into("<I", raw, 8, 4)
    bad = tmp_path / "bad.glcw"
    bad.write_bytes(bytes(raw))
    assert model.glc_weights_load(str(bad).encode(), C.byref(W)) != 0
    # the older writers: v2 / v3 / v4 headers carry nothing new
    for cname, ver, used in (("tiny", 2, 23), ("mb-tiny", 3, 26), ("q3-tiny", 4, 28)):
        p = str(tmp_path / (cname + ".glcw"))
        weights.write_blob(p, CONFIGS[cname], weights.make_weights(CONFIGS[cname], 7))
        with open(p, "rb") as f:
            hdr = f.read(256)
        assert struct.unpack_from("<I", hdr, 8)[0] == ver and hdr[16 + 4 * used:] == b"\x00" * (256 - 16 - 4 * used)
        c2, _ = weights.read_blob(p)
        assert (c2.max_positions, c2.type_vocab, c2.pos_offset) == (0, 0, 0)


def _hf_dir(tmp_path, cfg, tensors, model_type, prefix="encoder_model.", enc_extra=None, split=True):
    """an HF-layout directory: config.json + model.safetensors with query / key / value apart, as HF stores them"""
    from safetensors.numpy import save_file
    enc = dict(model_type=model_type, vocab_size=cfg.vocab - 2, hidden_size=cfg.hidden, intermediate_size=cfg.inter, num_hidden_layers=cfg.layers,
               num_attention_heads=cfg.heads, layer_norm_eps=cfg.ln_eps, hidden_act="gelu", position_embedding_type="absolute",
               max_position_embeddings=cfg.max_positions, type_vocab_size=cfg.type_vocab, pad_token_id=cfg.pad_id, cls_token_id=cfg.cls_id,
               sep_token_id=cfg.sep_id)
    enc.update(enc_extra or {})
    root = dict(encoder_config=enc, architecture_type="uni-encoder", scorer_type="simple", pooling_strategy="first",
                class_token_index=cfg.class_token_index, text_token_index=cfg.text_token_index, embed_class_token=True, normalize_features=False)
    d = tmp_path / f"ckpt_{len(list(tmp_path.iterdir()))}"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(root))
    sd = {}
    H = cfg.hidden
    for k, v in tensors.items():
        pre = prefix if "projector" not in k else ""
        if split and ".attention.self.Wqkv." in k:
            for i, part in enumerate(("query", "key", "value")):
                sd[pre + k.replace("Wqkv", part)] = np.ascontiguousarray(v[i * H:(i + 1) * H])
        else:
            sd[pre + k] = np.ascontiguousarray(v)
    sd[prefix + "pooler.dense.weight"] = np.zeros((H, H), np.float32)          # ignored
    save_file(sd, str(d / "model.safetensors"))
    return str(d)


@pytest.mark.parametrize("model_type,prefix", [("bert", "encoder_model."), ("roberta", "model.encoder_model."), ("xlm-roberta", ""), ("roberta", "roberta.")])
def test_checkpoint_import(libs, tmp_path, model_type, prefix):
    pytest.importorskip("safetensors")
    _lib, model = libs
    from gliclass.c_amd import weights
    from gliclass.c_amd.config import CONFIGS
    bert = model_type == "bert"
    cfg = dataclasses.replace(CONFIGS["bert-tiny"], layers=2, max_positions=90, pad_id=0 if bert else 1, pos_offset=0 if bert else 2, cls_id=5,
                              pos_buckets=0, max_rel_pos=0)
    ref = weights.make_weights(cfg, 4)
    path = _hf_dir(tmp_path, cfg, ref, model_type, prefix)
    pcfg, pt = weights.load_bert_checkpoint(path)                      # the Python importer
    assert dataclasses.replace(pcfg, name=cfg.name) == cfg
    assert list(pt) == list(ref) and all(np.array_equal(pt[n], ref[n]) for n in ref)
    W = _lib.Weights()
    assert model.glc_weights_load(path.encode(), C.byref(W)) == 0      # the C importer
    try:
        c = W.cfg
        for f in ("vocab", "hidden", "layers", "heads", "head_dim", "inter", "pad_id", "cls_id", "sep_id", "class_token_index", "text_token_index",
                  "backbone", "kv_heads", "causal", "pooling", "scorer", "embed_class_token", "normalize_features", "qk_norm", "attn_bias",
                  "max_positions", "type_vocab", "pos_offset"):
            assert getattr(c, f) == getattr(pcfg, f), f
        assert abs(c.ln_eps - cfg.ln_eps) < 1e-12
        specs = weights.tensor_specs(cfg)
        assert W.n_tensors == len(specs)
        for i, (n, shape, _, _) in enumerate(specs):
            assert np.array_equal(np.ctypeslib.as_array(W.tensors[i], shape=shape), ref[n]), n
        q = ref["encoder.layer.1.attention.self.Wqkv.weight"]
        got = np.ctypeslib.as_array(W.tensors[5 + 12], shape=q.shape)
        assert np.array_equal(got[128:256], q[128:256]) and not np.array_equal(got[:128], got[128:256])      # key rows behind the query rows
    finally:
        model.glc_weights_free(C.byref(W))


REFUSALS = [
    ({"position_embedding_type": "relative_key"}, "position_embedding_type 'relative_key' is not implemented"),
    ({"hidden_act": "relu"}, "hidden_act 'relu' is not implemented"),
    ({"is_decoder": True}, "is_decoder=true is not implemented"),
    ({"add_cross_attention": True}, "add_cross_attention=true is not implemented"),
    ({"num_attention_heads": 4}, "head_dim 32 is not implemented"),
    ({"max_position_embeddings": 2}, "max_position_embeddings 2 leaves no position behind the offset 2"),
]


@pytest.mark.parametrize("extra,msg", REFUSALS)
def test_checkpoint_rejections(libs, tmp_path, extra, msg):
    """Everything the engine does not build fails loudly, with a message that names the field: the C importer prints it to stderr
    (checked in a child), the Python importer raises it."""
    pytest.importorskip("safetensors")
    from gliclass.c_amd import weights
    from gliclass.c_amd.config import CONFIGS
    cfg = dataclasses.replace(CONFIGS["bert-tiny"], layers=1, max_positions=40)
    path = _hf_dir(tmp_path, cfg, weights.make_weights(cfg, 4), "roberta", "encoder_model.", extra)
    code = ("import ctypes as C, sys; sys.path.insert(0, %r); from gliclass.c_amd import _lib; W = _lib.Weights(); "
            "sys.exit(0 if _lib.model().glc_weights_load(%r, C.byref(W)) != 0 else 3)") % (ROOT, path.encode())
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    assert msg in r.stderr, r.stderr
    with pytest.raises(ValueError) as ei:
        weights.load_bert_checkpoint(path)
    assert msg in str(ei.value)


def test_unknown_model_type_names_the_family(libs, tmp_path):
    pytest.importorskip("safetensors")
    from gliclass.c_amd import weights
    from gliclass.c_amd.config import CONFIGS
    cfg = dataclasses.replace(CONFIGS["bert-tiny"], layers=1, max_positions=40)
    path = _hf_dir(tmp_path, cfg, weights.make_weights(cfg, 4), "electra")
    code = ("import ctypes as C, sys; sys.path.insert(0, %r); from gliclass.c_amd import _lib; W = _lib.Weights(); "
            "sys.exit(0 if _lib.model().glc_weights_load(%r, C.byref(W)) != 0 else 3)") % (ROOT, path.encode())
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "model_type 'electra' is not implemented" in r.stderr and "xlm-roberta" in r.stderr


def test_flops_per_seq():
    from gliclass.c_amd.config import CONFIGS
    cfg = CONFIGS["bert-base"]
    H, I, L = 768, 3072, 12
    for S, C_ in ((512, 4), (100, 1)):
        assert cfg.flops_per_seq(S, C_) == L * S * (8 * H * H + 4 * H * I + 4 * S * H) + 8 * H * H * (1 + C_)
