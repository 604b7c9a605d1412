"""GPU (-m gpu): the opt-in MX pipeline for forwards below the 256 tile's fill rule (glc_engine_set_mx_small_forwards / GLICLASS_MX_SMALL;
engine.hip run_forward_deberta, GemmGs; the 128 tile of csrc/gemm128x.hip).

What holds without a tolerance: with the switch at 0 nothing changes (the forward is the one an engine with nothing set runs); with it on, a
taken forward equals, bit for bit, the 256-tile MX forward of the same shape (glc_debug_set_group_split(2)) — the 128 tile adds the same
products in the same order (tests/test_gpu_gemm128x.py).  Against the split-f16 arithmetic the probabilities move by the MX arithmetic's
error: TOL_MX = 5e-4 of the existing MX tests (test_gpu_mx.py, test_gpu_parity.py); against the oracle at small 8 x 512 the bar is the 3e-4
test_gpu_fullsize.py holds MX forwards to."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL_MX = 5e-4
sig = lambda x: 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def _engine(weights_for, cname="mini", w=None):
    from gliclass.c_amd.engine import Engine
    cfg, w0 = weights_for(cname)
    eng = Engine(cfg, w if w is not None else w0, dtype="f32")
    eng.set_length_buckets(1)
    return cfg, eng


def _inputs(cfg, B, S, Cn, ragged=True):
    from gliclass.c_amd import synth
    ids, mask, _ = synth.make_inputs(cfg, B, S, Cn, seed=B + S, ragged=ragged)
    return ids, mask


@pytest.mark.parametrize("B,S", ((3, 100), (1, 64), (5, 330)))
def test_default_unchanged_and_mode_2_equals_the_256_tile_forward(weights_for, B, S):
    cfg, eng = _engine(weights_for)
    try:
        ids, mask = _inputs(cfg, B, S, 3)
        ref = eng.forward(ids, mask)                            # nothing set: the split-f16 kernels of a small forward
        assert not eng.last_mx() and eng.last_mx128() == 0 and not eng.last_group_split()
        eng.set_mx_small_forwards(0)
        assert np.array_equal(eng.forward(ids, mask), ref) and not eng.last_mx() and eng.last_mx128() == 0
        eng.set_mx_small_forwards(2)
        got = eng.forward(ids, mask)
        assert eng.last_mx() and eng.last_mx128() > 0, eng.last_mx128()
        n128 = eng.last_mx128()
        eng.set_mx_small_forwards(0)
        eng.set_group_split(2)                                  # the MX forward of the same shape on the 256 tile
        on256 = eng.forward(ids, mask)
        assert eng.last_mx() and eng.last_mx128() == 0
        assert np.array_equal(got, on256), "the 128-tile forward differs from the 256-tile MX forward"
        d = float(np.abs(sig(got) - sig(ref)).max())
        print(f"[mx_small] mini B={B} S={S}: {n128} launches on the 128 tile, max |prob - split-f16 prob| = {d:.2e}")
        assert np.isfinite(got).all() and d <= TOL_MX and not np.array_equal(got, ref), d
        eng.set_group_split(1)
        assert np.array_equal(eng.forward(ids, mask), ref) and eng.last_mx128() == 0      # ... and everything off again: the first forward
    finally:
        eng.close()


def _device_cus(eng):
    import gemm_ref as R
    from gemm_run import run
    res = run(eng, 5, R.EPI_BIAS, np.zeros((128, 32), np.float32), np.zeros((128, 32), np.float32))
    assert res["rc"] == 0, res["err"]
    return res["cus"]


def test_mode_1_follows_the_fill_rule_of_the_128_tile(weights_for):
    cfg, eng = _engine(weights_for)
    _, plain = _engine(weights_for)
    try:
        cus = _device_cus(eng)
        H = cfg.hidden
        eng.set_mx_small_forwards(1)
        for (B, S, taken_on_256_cus) in ((16, 512, True), (1, 128, False)):
            Sp = -(-S // 64) * 64
            Mpad = -(-(B * Sp) // 256) * 256
            small256 = (Mpad // 256) * (H // 256) * 2 < cus      # glc_gemm_small_m: not enough 256-tiles
            fill128 = (Mpad // 128) * (H // 128) * 2 >= cus
            expect = small256 and fill128
            if cus == 256:
                assert expect == taken_on_256_cus
            ids, mask = _inputs(cfg, B, S, 3)
            got = eng.forward(ids, mask)
            print(f"[mx_small] mode 1, {cus} CUs, mini B={B} S={S}: expected taken = {expect}, launches on the 128 tile = {eng.last_mx128()}")
            assert (eng.last_mx128() > 0) == expect and eng.last_mx() == (expect or not small256)
            if not expect and small256:                         # not taken: the forward of an engine with nothing set
                assert np.array_equal(got, plain.forward(ids, mask))
    finally:
        eng.close()
        plain.close()


def test_small_8x512_against_the_oracle(weights_for):
    import oracle_c
    cfg, eng = _engine(weights_for, "small")
    try:
        ids, mask = _inputs(cfg, 8, 512, 8, ragged=False)
        eng.set_mx_small_forwards(1)
        got = eng.forward(ids, mask)
        cus = _device_cus(eng)
        expect = (4096 // 256) * 3 * 2 < cus and (4096 // 128) * 6 * 2 >= cus
        assert (eng.last_mx128() > 0) == expect and eng.last_mx() == expect, (cus, eng.last_mx128())
        _, w = weights_for("small")
        ref = oracle_c.forward(cfg, w, ids, mask)
        err = float(np.abs(sig(got) - sig(ref)).max())
        print(f"[mx_small] small 8 x 512, mode 1 ({eng.last_mx128()} launches on the 128 tile): max |prob - oracle| = {err:.2e}")
        assert np.isfinite(got).all() and err <= 3e-4, err
    finally:
        eng.close()


def test_device_resident_range_report_in_mode_2(weights_for):
    """the construction of test_fp8_range_guard_device_resident_forward_contract (test_gpu_mx.py) on mini at B = 3, S = 100: one channel of
    every attention-output bias at 600 puts raw residual rows beyond the e4m3 range; a device-resident forward taken by the switch is reported
    by glc_engine_sync, the engine lowers the rows' exponent, the repeat is valid and equals the host-buffer forward"""
    cfg, w0 = weights_for("mini")
    w = dict(w0)
    for name in list(w):
        if name.endswith("attention.output.dense.bias"):
            bvec = w[name].copy(); bvec[77] = 600.0; w[name] = bvec
    B, S, Cn = 3, 100, 3
    ids, mask = _inputs(cfg, B, S, Cn)
    _, ref_eng = _engine(weights_for, w=w)
    try:
        ref_eng.set_mx_small_forwards(2)
        assert ref_eng.activation_exponent() == 0
        want = ref_eng.forward(ids, mask)                       # host-buffer forward: repeats itself at exponent -5, still on the MX pipeline
        assert ref_eng.last_mx() and ref_eng.last_mx128() > 0 and ref_eng.activation_exponent() == -5 and ref_eng.fp8_range_retries() == 1
    finally:
        ref_eng.close()
    _, eng = _engine(weights_for, w=w)
    bufs = []
    try:
        eng.set_mx_small_forwards(2)
        d_ids, d_mask, d_out = eng.dev_alloc(ids.nbytes), eng.dev_alloc(mask.nbytes), eng.dev_alloc(B * Cn * 4)
        bufs = [d_ids, d_mask, d_out]
        eng.h2d(d_ids, ids.astype(np.int64)); eng.h2d(d_mask, mask.astype(np.int64))
        eng.forward_device(d_ids, d_mask, B, S, Cn, d_out)
        assert eng.last_mx128() > 0
        assert eng.L.glc_engine_sync(eng.h) == -1 and b"run the forward again" in eng.L.glc_last_error()
        assert eng.activation_exponent() == -5 and not eng.fp8_range_sticky()
        eng.forward_device(d_ids, d_mask, B, S, Cn, d_out)
        eng.sync()
        out = np.zeros((B, Cn), np.float32)
        eng.d2h(out, d_out)
        assert eng.last_mx128() > 0 and np.array_equal(out, want)
    finally:
        for p in bufs:
            eng.dev_free(p)
        eng.close()


def test_graph_replay_in_mode_2(weights_for):
    cfg, eager = _engine(weights_for)
    _, replay = _engine(weights_for)
    try:
        ids, mask = _inputs(cfg, 3, 100, 3)
        eager.set_mx_small_forwards(2)
        want = eager.forward(ids, mask)
        replay.set_graph_replay(True)
        replay.set_mx_small_forwards(2)
        states = []
        for _ in range(3):
            got = replay.forward(ids, mask)
            states.append(replay.last_graph())
            assert np.array_equal(got, want) and replay.last_mx() and replay.last_mx128() == eager.last_mx128() > 0
        assert states == [0, 1, 2], states
        replay.set_mx_small_forwards(0)                         # changing the mode drops the cached graphs
        assert replay.graph_cache_size() == 0
    finally:
        eager.close()
        replay.close()


@pytest.mark.parametrize("cname,word", (("dec-tiny", "decoder"), ("mb-mini", "modernbert")))
def test_other_backbones_refuse_the_switch(weights_for, cname, word):
    _, eng = _engine(weights_for, cname)
    try:
        assert eng.L.glc_engine_set_mx_small_forwards(eng.h, 1) == -1 and word in eng.L.glc_last_error().decode().lower()
        with pytest.raises(Exception):
            eng.set_mx_small_forwards(2)
        eng.set_mx_small_forwards(0)
        assert eng.last_mx128() == 0
    finally:
        eng.close()
