"""T5 / mT5 backbone, host side (no GPU): the float64 restatement against the committed HF fixtures, the exported bucket function
against torch's, the C config / tensor-spec mirror, the v6 blob header, and the checkpoint importers (C and Python) with their refusals."""
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

import t5_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
T5_CONFIGS = ("t5-tiny", "t5-odd", "t5-mini", "t5-base")
CASES = ("tiny_s1", "tiny_s33", "tiny_s130", "odd_rpad", "odd_lpad")
CFG_FIELDS = ("vocab", "hidden", "layers", "heads", "head_dim", "inter", "pad_id", "cls_id", "sep_id", "class_token_index", "text_token_index",
              "backbone", "kv_heads", "causal", "pooling", "scorer", "embed_class_token", "normalize_features", "qk_norm", "attn_bias",
              "max_positions", "type_vocab", "pos_offset", "rel_buckets", "rel_max_distance")


@pytest.fixture(scope="module")
def libs():
    from gliclass.c_amd import _lib
    return _lib, _lib.model()


def test_fixture_set_is_complete():
    files = glob.glob(os.path.join(GOLDEN, "t5", "*.npz"))
    assert {os.path.basename(f)[:-4] for f in files} == set(CASES) | {"t5-tiny_weights", "t5-odd_weights", "buckets"}
    assert all(os.path.getsize(f) < 900 * 1024 for f in files)


@pytest.mark.parametrize("case", CASES)
def test_reference_matches_fixtures(case):
    z = np.load(os.path.join(GOLDEN, "t5", case + ".npz"))
    cfg, t = t5_ref.fixture_model(GOLDEN, str(z["flavour"]))
    ids, mask = z["ids"].astype(np.int64), z["mask"].astype(np.int64)
    hs = t5_ref.backbone(cfg, t, ids, mask)
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
        assert ids.shape[1] > 128          # (distance 129 lies beyond relative_attention_max_distance)
    if ids.shape[1] > 1:                   # the fixtures see the bias
        assert np.abs(t5_ref.backbone(cfg, t, ids, mask, zero_bias=True)[-1] - hs[-1])[mask.astype(bool)].max() > 0.1


def test_fixture_weights_are_not_defaults():
    for flavour, nh in (("t5-tiny", 2), ("t5-odd", 3)):
        cfg, t = t5_ref.fixture_model(GOLDEN, flavour)
        assert (cfg.heads, cfg.hidden, cfg.heads * cfg.head_dim != cfg.hidden) == (nh, 128, nh == 3)
        rb = t["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"]
        assert rb.shape == (32, nh) and rb.std() > 1.0
        for n, v in t.items():
            if n.endswith("layer_norm.weight"):
                assert np.abs(v - 1).max() > 0.1, n


@pytest.mark.parametrize("nb,md", [(32, 128), (8, 20)])
def test_bucket_function_bit_exact(libs, nb, md):
    """glc_t5_bucket_table against torch's T5Attention._relative_position_bucket (bidirectional) for every delta in [-4095, 4095]:
    (32, 128) from the committed buckets.npz, (8, 20) computed live; t5_ref.bucket restates the same float32 steps.  At (32, 128) a
    float64 evaluation of the log branch agrees with torch's float32 at every delta of the range (checked here too): the integer points
    of the log spacing, |delta| = 16, 32, 64, come out exact in both."""
    from gliclass.c_amd.engine import t5_bucket_table
    delta = np.arange(-4095, 4096)
    if nb == 32:
        z = np.load(os.path.join(GOLDEN, "t5", "buckets.npz"))
        assert (int(z["num_buckets"]), int(z["max_distance"])) == (nb, md) and np.array_equal(z["delta"], delta)
        want = z["bucket"].astype(np.int64)
    else:
        import torch
        from transformers.models.t5.modeling_t5 import T5Attention
        want = T5Attention._relative_position_bucket(torch.from_numpy(delta), True, nb, md).numpy()
    got = t5_bucket_table(4096, nb, md)
    assert got.shape == (8191,) and np.array_equal(got, want)
    assert np.array_equal(t5_ref.bucket(delta, nb, md), want)
    assert got.min() == 0 and got.max() == nb - 1 and got[4095] == 0 and got[4095 + 1] == nb // 2 + 1 and got[4095 - 1] == 1
    if nb == 32:
        half, me = 16, 8
        a = np.abs(delta).astype(np.float64)
        big = me + np.floor(np.log(np.maximum(a, 1) / me) / np.log(md / me) * (half - me)).astype(np.int64)
        f64 = np.where(delta > 0, half, 0) + np.where(a < me, a.astype(np.int64), np.minimum(big, half - 1))
        assert np.array_equal(f64, want)


def test_named_configs_and_tensor_specs_match_python(libs):
    _lib, model = libs
    from gliclass.c_amd import weights
    from gliclass.c_amd.config import CONFIGS, BACKBONE_T5
    for cname in T5_CONFIGS:
        cfg = CONFIGS[cname]
        assert cfg.backbone == BACKBONE_T5 == 4 and cfg.head_dim == 64 and (cfg.rel_buckets, cfg.rel_max_distance) == (32, 128)
        cc = _lib.ModelConfig()
        assert model.glc_named_config(cname.encode(), C.byref(cc)) == 0
        assert abs(cc.ln_eps / cfg.ln_eps - 1) < 1e-6
        for f in CFG_FIELDS + ("pos_buckets", "max_rel_pos"):
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
        assert len(specs) == 2 + 6 * cfg.layers + 1 + 8
    t, o, m, b = (CONFIGS[n] for n in T5_CONFIGS)
    assert (t.hidden, t.heads, t.inter, t.layers) == (128, 2, 256, 2) and (o.hidden, o.heads) == (128, 3)
    assert (m.hidden, m.heads, m.inter) == (256, 4, 512) and (b.hidden, b.heads, b.inter, b.layers, b.vocab) == (768, 12, 2048, 12, 32128)


def test_synthetic_weights_bit_identical_to_python(libs, c_generated_weights):
    from gliclass.c_amd import weights
    from gliclass.c_amd.config import CONFIGS
    cfg = CONFIGS["t5-odd"]
    ref = weights.make_weights(cfg, 9)
    got = c_generated_weights("synthetic:t5-odd:9", cfg)
    assert list(got) == list(ref) and all(np.array_equal(got[k], ref[k]) for k in ref)


def test_blob_v6_round_trip_and_older_headers_unchanged(libs, tmp_path):
    _lib, model = libs
    from gliclass.c_amd import weights
    from gliclass.c_amd.config import CONFIGS
    cfg = dataclasses.replace(CONFIGS["t5-odd"], rel_buckets=8, rel_max_distance=20)
    ref = weights.make_weights(cfg, 7)
    path = str(tmp_path / "t5.glcw")
    weights.write_blob(path, cfg, ref)
    with open(path, "rb") as f:
        hdr = f.read(256)
    assert struct.unpack_from("<I", hdr, 8)[0] == 6
    assert struct.unpack_from("<5i", hdr, 16 + 4 * 28) == (0, 0, 0, 8, 20) and hdr[16 + 4 * 33:] == b"\x00" * (256 - 16 - 4 * 33)
    cfg2, back = weights.read_blob(path)
    assert dataclasses.replace(cfg2, name=cfg.name, ln_eps=cfg.ln_eps) == cfg and abs(cfg2.ln_eps / cfg.ln_eps - 1) < 1e-6
    assert all(np.array_equal(back[n], ref[n]) for n in ref)
    W = _lib.Weights()
    assert model.glc_weights_load(path.encode(), C.byref(W)) == 0
    try:
        assert (W.cfg.backbone, W.cfg.heads, W.cfg.rel_buckets, W.cfg.rel_max_distance) == (4, 3, 8, 20)
        assert W.n_tensors == len(ref)
        for i, (n, shape, _, _) in enumerate(weights.tensor_specs(cfg)):
            assert np.array_equal(np.ctypeslib.as_array(W.tensors[i], shape=shape), ref[n])
    finally:
        model.glc_weights_free(C.byref(W))
    # a T5 blob under an older version is refused
    raw = bytearray(open(path, "rb").read())
    struct.pack_into("<I", raw, 8, 5)
    bad = tmp_path / "bad.glcw"
    bad.write_bytes(bytes(raw))
    assert model.glc_weights_load(str(bad).encode(), C.byref(W)) != 0
    # the older writers: v2 - v5 headers carry nothing new
    for cname, ver, used in (("tiny", 2, 23), ("mb-tiny", 3, 26), ("q3-tiny", 4, 28), ("bert-tiny", 5, 31)):
        p = str(tmp_path / (cname + ".glcw"))
        weights.write_blob(p, CONFIGS[cname], weights.make_weights(CONFIGS[cname], 7))
        with open(p, "rb") as f:
            hdr = f.read(256)
        assert struct.unpack_from("<I", hdr, 8)[0] == ver and hdr[16 + 4 * used:] == b"\x00" * (256 - 16 - 4 * used)
        c2, _ = weights.read_blob(p)
        assert (c2.rel_buckets, c2.rel_max_distance) == (0, 0)
        assert model.glc_weights_load(p.encode(), C.byref(W)) == 0
        try:
            assert (W.cfg.rel_buckets, W.cfg.rel_max_distance) == (0, 0)
        finally:
            model.glc_weights_free(C.byref(W))


def _hf_dir(tmp_path, cfg, tensors, model_type, prefix="encoder_model.", enc_extra=None, tied_name="shared.weight", encoder=True):
    """an HF-layout directory: config.json + model.safetensors with q / k / v and wi_0 / wi_1 apart, as HF stores them, and a few
    decoder-side tensors the importers must ignore"""
    from safetensors.numpy import save_file
    enc = dict(model_type=model_type, vocab_size=cfg.vocab - 2, d_model=cfg.hidden, d_ff=cfg.inter, num_layers=cfg.layers, num_heads=cfg.heads,
               d_kv=cfg.head_dim, layer_norm_epsilon=cfg.ln_eps, feed_forward_proj="gated-gelu", dense_act_fn="gelu_new",
               relative_attention_num_buckets=cfg.rel_buckets, relative_attention_max_distance=cfg.rel_max_distance,
               pad_token_id=cfg.pad_id, cls_token_id=cfg.cls_id, sep_token_id=cfg.sep_id)
    enc.update(enc_extra or {})
    root = dict(encoder_config=enc, architecture_type="uni-encoder", scorer_type="simple", pooling_strategy="first",
                class_token_index=cfg.class_token_index, text_token_index=cfg.text_token_index, embed_class_token=True, normalize_features=False)
    d = tmp_path / f"ckpt_{len(list(tmp_path.iterdir()))}"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(root))
    sd = {}
    inner, I = cfg.heads * cfg.head_dim, cfg.inter
    for k, v in tensors.items():
        pre = prefix if "projector" not in k else ""
        if ".SelfAttention.Wqkv." in k:
            for i, part in enumerate(("q", "k", "v")):
                sd[pre + k.replace("Wqkv", part)] = np.ascontiguousarray(v[i * inner:(i + 1) * inner])
        elif ".DenseReluDense.Wgu." in k:
            for i, part in enumerate(("wi_0", "wi_1")):
                sd[pre + k.replace("Wgu", part)] = np.ascontiguousarray(v[i * I:(i + 1) * I])
        elif k == "shared.weight":
            sd[pre + tied_name] = np.ascontiguousarray(v)
        else:
            sd[pre + k] = np.ascontiguousarray(v)
    if not encoder:
        sd = {k.replace("encoder.block", "decoder.block"): v for k, v in sd.items()}
    sd[prefix + "decoder.block.0.layer.1.EncDecAttention.q.weight"] = np.zeros((inner, cfg.hidden), np.float32)      # ignored
    sd[prefix + "lm_head.weight"] = np.zeros((4, cfg.hidden), np.float32)                                            # ignored
    save_file(sd, str(d / "model.safetensors"))
    return str(d)


@pytest.mark.parametrize("model_type,prefix,tied", [("t5", "encoder_model.", "shared.weight"), ("mt5", "model.encoder_model.", "shared.weight"),
                                                    ("t5", "", "encoder.embed_tokens.weight"), ("mt5", "model.", "shared.weight")])
def test_checkpoint_import(libs, tmp_path, model_type, prefix, tied):
    pytest.importorskip("safetensors")
    _lib, model = libs
    from gliclass.c_amd import weights
    from gliclass.c_amd.config import CONFIGS
    cfg = dataclasses.replace(CONFIGS["t5-odd"], cls_id=5)
    ref = weights.make_weights(cfg, 4)
    path = _hf_dir(tmp_path, cfg, ref, model_type, prefix, tied_name=tied)
    pcfg, pt = weights.load_t5_checkpoint(path)                        # the Python importer
    assert dataclasses.replace(pcfg, name=cfg.name) == cfg
    assert list(pt) == list(ref) and all(np.array_equal(pt[n], ref[n]) for n in ref)
    W = _lib.Weights()
    assert model.glc_weights_load(path.encode(), C.byref(W)) == 0      # the C importer
    try:
        for f in CFG_FIELDS:
            assert getattr(W.cfg, f) == getattr(pcfg, f), f
        assert abs(W.cfg.ln_eps - cfg.ln_eps) < 1e-12
        specs = weights.tensor_specs(cfg)
        assert W.n_tensors == len(specs)
        for i, (n, shape, _, _) in enumerate(specs):
            assert np.array_equal(np.ctypeslib.as_array(W.tensors[i], shape=shape), ref[n]), n
        q = ref["encoder.block.1.layer.0.SelfAttention.Wqkv.weight"]
        got = np.ctypeslib.as_array(W.tensors[2 + 6 + 1], shape=q.shape)
        assert np.array_equal(got[192:384], q[192:384]) and not np.array_equal(got[:192], got[192:384])      # key rows behind the query rows
    finally:
        model.glc_weights_free(C.byref(W))


REFUSALS = [
    ({"feed_forward_proj": "relu"}, "feed_forward_proj 'relu' is not implemented"),
    ({"d_kv": 32}, "d_kv 32 is not implemented"),
    ({"is_decoder": True}, "is_decoder=true is not implemented"),
    ({"model_type": "umt5"}, "model_type 'umt5' is not implemented"),
    ({"dense_act_fn": "gelu"}, "dense_act_fn 'gelu' is not implemented"),
]


def _c_load_stderr(path):
    code = ("import ctypes as C, sys; sys.path.insert(0, %r); from gliclass.c_amd import _lib; W = _lib.Weights(); "
            "sys.exit(0 if _lib.model().glc_weights_load(%r, C.byref(W)) != 0 else 3)") % (ROOT, path.encode())
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    return r.stderr


@pytest.mark.parametrize("extra,msg", REFUSALS)
def test_checkpoint_rejections(libs, tmp_path, extra, msg):
    """Everything the engine does not build fails loudly, with a message that names the field: the C importer prints it to stderr
    (checked in a child), the Python importer raises it."""
    pytest.importorskip("safetensors")
    from gliclass.c_amd import weights
    from gliclass.c_amd.config import CONFIGS
    cfg = dataclasses.replace(CONFIGS["t5-tiny"], layers=1)
    path = _hf_dir(tmp_path, cfg, weights.make_weights(cfg, 4), "t5", "encoder_model.", extra)
    assert msg in _c_load_stderr(path)
    with pytest.raises(ValueError) as ei:
        weights.load_t5_checkpoint(path)
    assert msg in str(ei.value)


def test_checkpoint_without_encoder_tensors_is_refused(libs, tmp_path):
    """an is_decoder / is_encoder_decoder-only checkpoint: decoder blocks, no encoder.block tensors"""
    pytest.importorskip("safetensors")
    from gliclass.c_amd import weights
    from gliclass.c_amd.config import CONFIGS
    cfg = dataclasses.replace(CONFIGS["t5-tiny"], layers=1)
    path = _hf_dir(tmp_path, cfg, weights.make_weights(cfg, 4), "t5", "encoder_model.", {"is_encoder_decoder": True}, encoder=False)
    msg = "is_encoder_decoder: the checkpoint holds no encoder tensors"
    assert msg in _c_load_stderr(path)
    with pytest.raises(ValueError) as ei:
        weights.load_t5_checkpoint(path)
    assert msg in str(ei.value)


def test_unknown_model_type_names_the_family(libs, tmp_path):
    pytest.importorskip("safetensors")
    from gliclass.c_amd import weights
    from gliclass.c_amd.config import CONFIGS
    cfg = dataclasses.replace(CONFIGS["t5-tiny"], layers=1)
    path = _hf_dir(tmp_path, cfg, weights.make_weights(cfg, 4), "electra",
                   enc_extra=dict(hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256))
    err = _c_load_stderr(path)
    assert "model_type 'electra' is not implemented" in err and "xlm-roberta, t5, mt5)" in err


def test_flops_per_seq():
    from gliclass.c_amd.config import CONFIGS
    cfg = CONFIGS["t5-odd"]
    H, I, L, nqd = 128, 256, 2, 192
    for S, C_ in ((512, 4), (100, 1)):
        assert cfg.flops_per_seq(S, C_) == L * S * (8 * H * nqd + 6 * H * I + 4 * S * nqd) + 8 * H * H * (1 + C_)
