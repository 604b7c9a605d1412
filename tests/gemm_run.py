"""One glc_debug_gemm_run call (include/gliclass_hip.h) from numpy operands: the helper the GPU kernel tests share
(tests/test_gpu_gemm_kernels.py, tests/test_gpu_mx.py).  The entry returns raw bytes only; tests/gemm_ref.py decodes them."""
import ctypes as C

import numpy as np

import gemm_ref as R

FILL = 0xA5


def out_bytes(kernel, epi, dt, Mpad, N, Mvalid=0, Sp=0, nh=0, nq=0, nkv=0):
    es = 4 if kernel in (R.KGS, R.KMX) or dt == "f32" else 2
    if epi == R.EPI_QKV:
        B = -(-min(Mvalid, Mpad) // Sp)
        return [B * nh * Sp * 64 * es] * 3
    if epi == R.EPI_QKVR:
        B = -(-min(Mvalid, Mpad) // Sp)
        return [B * nq * Sp * 512, B * nkv * Sp * 512, B * nkv * Sp * 512]
    return [Mpad * (N // 2 if epi in (R.EPI_SWIGLU, R.EPI_GEGLU) else N) * es, 0, 0]


def run(eng, kernel, epi, A, W, **o):
    """One glc_debug_gemm_run call -> dict(rc, err, out [3 x uint8], ln_part, A_img, W_img, W2_img, resid_img, sat, guards_ok)."""
    from gliclass.c_amd import _lib
    r = _lib.GemmRun()
    keep = []

    def fp(x):
        if x is None:
            return None
        a = np.ascontiguousarray(x, np.float32)
        keep.append(a)
        return a.ctypes.data_as(C.POINTER(C.c_float))
    Mpad, K = (o.pop("Mpad", None) or A.shape[0]), (o.pop("K", None) or A.shape[1])
    N = o.pop("N", None) or W.shape[0]
    r.kernel, r.epi, r.Mpad, r.N, r.K = kernel, epi, Mpad, N, K
    r.A, r.W = fp(A), fp(W)
    for name in ("bias", "W2", "bias2", "resid", "a_stats", "ln_c", "r_stats", "r_gamma", "r_beta", "rope_cs"):
        if o.get(name) is not None:
            setattr(r, name, fp(o.pop(name)))
        else:
            o.pop(name, None)
    flags = o.pop("q_tile_flag", None)
    if flags is not None:
        flags = np.ascontiguousarray(flags, np.uint8); keep.append(flags); r.q_tile_flag = flags.ctypes.data
    r.qscale = o.pop("qscale", 1.0)
    r.fill = FILL
    r.ws_bytes = o.pop("ws_bytes", 0)
    sizes = o.pop("out_bytes", None) or out_bytes(kernel, epi, eng.dtype, Mpad, N, o.get("Mvalid", 0), o.get("Sp", 0), o.get("nh", 0), o.get("nq", 0), o.get("nkv", 0))
    for name in list(o):
        setattr(r, name, int(o.pop(name)))
    es = 4 if kernel in (R.KGS, R.KMX) or eng.dtype == "f32" else 2
    outs = [np.zeros(max(int(s), 1), np.uint8) for s in sizes]
    for i in range(3):
        r.out[i] = outs[i].ctypes.data
        r.out_bytes[i] = int(sizes[i])
    imgs = {"A_img": np.zeros(Mpad * K * es, np.uint8), "W_img": np.zeros(N * K * es, np.uint8), "W2_img": np.zeros(N * K * es, np.uint8),
            "resid_img": np.zeros(Mpad * N * 4, np.uint8)}
    for k, v in imgs.items():
        setattr(r, k, v.ctypes.data)
    lp = np.zeros((Mpad, max(N // 64, 1), 2), np.float32)
    r.ln_part = lp.ctypes.data
    rc = eng.L.glc_debug_gemm_run(eng.h, C.byref(r))
    return dict(rc=rc, err=eng.L.glc_last_error().decode() if rc else "", out=[outs[i][:int(sizes[i])] for i in range(3)], ln_part=lp, sat=(r.sat[0], r.sat[1]),
                guards_ok=r.guards_ok, cus=r.cus, es=es, **imgs)
