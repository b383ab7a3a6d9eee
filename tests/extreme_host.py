"""What the tests on tests/extreme_blocks.py share on the host: the recorded truth (tests/golden/extreme_blocks.npz, written by
`python oracle/gen_golden.py extremes` from both reference builds), a CPU weight quantizer for the `quantizer` family (the oracle's
for the legacy formats; for the k-quants, which the oracle does not restate, the host build of csrc/fq_wquant.h that
tests/test_wquant_cpu.py pins to the reference's vectors), and the case's inputs checked against their recorded sha256."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np

from oracle import binding as ob
import extreme_blocks as xb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZERO_ROW = xb.ACT_ROWS.index("zero")
NEG_ZERO = np.uint32(0x80000000)
_cache = {}


def golden():
    if "g" not in _cache:
        with np.load(os.path.join(ROOT, "tests", "golden", "extreme_blocks.npz")) as z:
            _cache["g"] = {k: z[k] for k in z.files}
    return _cache["g"]


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def cpu_quantizer(oracle):
    """quantize(t, x[M, K]) -> [M, row_bytes] on the CPU"""
    if "wq" not in _cache:
        src = os.path.join(ROOT, "tests", "host", "wquant_harness.cpp")
        out = os.path.join(ROOT, "tests", "host", "libwquant_host.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "ggllm.cpp_amd", "csrc"), "-o", out, src])
        L = C.CDLL(out)
        L.wquant_rows.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        _cache["wq"] = L
    L = _cache["wq"]

    def quantize(t, x):
        x = np.ascontiguousarray(x, np.float32)
        if t in ob.LEGACY:
            return np.stack([oracle.quantize(t, row) for row in x])
        out = np.zeros((x.shape[0], ob.row_bytes(t, x.shape[1])), np.uint8)
        for r in range(x.shape[0]):
            assert L.wquant_rows(t, x[r].ctypes.data, x.shape[1], out[r].ctypes.data, None) == 0
        return out
    return quantize


def activations(K):
    """the 16 activation rows at width K, the very bytes the fixture was recorded on"""
    if ("x", K) not in _cache:
        A = xb.activations(K, xb.SEED)
        assert np.array_equal(sha(A), golden()[f"x_{K}_sha256"]), "tests/extreme_blocks.py no longer generates the recorded activations"
        A.setflags(write=False)
        _cache["x", K] = A
    return _cache["x", K]


def case_weights(name, t, fam, K, quantize, M=xb.M_ROWS):
    """the case's weight bytes, the very bytes the fixture was recorded on (the `quantizer` family: `quantize` reproduces the reference's quantizer)"""
    w = xb.weights(t, fam, M, K, xb.SEED, quantize=quantize)
    assert np.array_equal(sha(w), golden()[f"{name}_w_sha256"]), f"{name}: the weight bytes differ from the recorded ones"
    return w


def oracle_mul_mat(oracle, order, t, w, K, x):
    oracle.lib.orc_set_sum_order(order)
    try:
        return oracle.mul_mat(t, w, K, w.shape[0], x, 4)
    finally:
        oracle.lib.orc_set_sum_order(0)


def act_image(oracle, t, x):
    """the oracle's Q8_0 / Q8_1 / Q8_K image of the rows x (the reference's scalar rounding)"""
    return np.stack([oracle.quantize_act(ob.VEC_DOT[t], row) for row in x])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bound(name):
    """the term-magnitude bound of a case: 4 x the larger of the two reference builds' recorded errors. The kernels' orders differ from the reference's in
    association only; a dropped or doubled term moves extreme_blocks.term_error by 1e-3 or more."""
    return 4.0 * float(golden()[f"{name}_err"].max())
