"""Developer tool (GPU): the MX cross-term GEMM (gemm256x.hip) against the split-f16 GEMM — timing.  The numerics of the pair are a test."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gliclass.c_amd.config import CONFIGS
from gliclass.c_amd import weights
from gliclass.c_amd.engine import Engine
print("numerics (every epilogue, MX against split-f16 on the same operands): python -m pytest tests/test_gpu_mx.py -m gpu -s -k test_mx_gemm_every_epilogue_vs_split_gemm", flush=True)
e = Engine(CONFIGS["tiny"], weights.make_weights(CONFIGS["tiny"], 1), dtype="f16")
EPI = {"bias": 0, "gelu": 1, "resid": 2}
M = 65536
shapes = [("attn-out", M, 768, 768, "resid"), ("ffn1", M, 3072, 768, "gelu"), ("ffn2", M, 768, 3072, "resid"), ("qkv-as-bias", M, 2304, 768, "bias")]
for rnd in range(2):
    for (name, M_, N, K, ep) in shapes:
        r = {}
        for which in (6, 9):
            r[which] = e.L.glc_debug_gemm_bench(e.h, M_, N, K, EPI[ep], 10, which)
        print(f"r{rnd} {name:12s} split-f16 {r[6]*1e3:7.1f} us   MX {r[9]*1e3:7.1f} us  ({r[6]/r[9]:.3f}x)  {2.0*M_*N*K/r[9]/1e9:7.1f} TF fp32-equivalent", flush=True)
e.close()
