"""Shared by tests/test_score_cpu.py and tests/test_gpu_score.py: the host harness (tests/host/score_harness.cpp, built with
g++) and the input sets of the scoring tests -- fixed seeds, so both files see the same rows."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V_MODEL = 65024             # Falcon-7B's vocabulary
V_ODD = 4099                # set (d): one chain tile of the kernel (4096) plus 3 -- no multiple of the tile, of 4 or of the wave


def build_harness(tmp_dir):
    so = os.path.join(str(tmp_dir), "libscore_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I",
                           os.path.join(ROOT, "ggllm.cpp_amd", "csrc"), "-o", so, os.path.join(ROOT, "tests", "host", "score_harness.cpp")])
    H = C.CDLL(so)
    for f in (H.score_fq, H.score_libm):
        f.restype = None
        f.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return H


def host_score(fn, rows, targets, V=None, want_terms=False):
    """fn: H.score_fq / H.score_libm over rows [R][stride >= V] (row r's logits in [:V]; V None: the whole row); returns prob f32, max f32, sum f64
    (entries of rows with a target < 0 keep the NaN they start with) and, with want_terms, the rows' expf terms [R][V]"""
    rows = np.ascontiguousarray(rows, np.float32)
    R, S = rows.shape
    V = S if V is None else V
    tg = np.ascontiguousarray(targets, np.int32)
    assert tg.shape == (R,) and int(tg.max(initial=-1)) < V
    prob, mx, sm = np.full(R, np.nan, np.float32), np.full(R, np.nan, np.float32), np.full(R, np.nan, np.float64)
    terms = np.zeros((R, V), np.float32) if want_terms else None
    fn(rows.ctypes.data, S, R, V, tg.ctypes.data, prob.ctypes.data, mx.ctypes.data, sm.ctypes.data, terms.ctypes.data if want_terms else None)
    return (prob, mx, sm, terms) if want_terms else (prob, mx, sm)


def set_a():
    """V = 65 024, 16 rows N(0, 8^2)"""
    return (np.random.default_rng(65024).standard_normal((16, V_MODEL)) * 8.0).astype(np.float32)


def set_b():
    """V = 333: 32 rows N(0, 8^2) (seed 341) and 32 rows uniform over [-40, 0] (seed 373)"""
    n = (np.random.default_rng(341).standard_normal((32, 333)) * 8.0).astype(np.float32)
    u = np.random.default_rng(373).uniform(-40.0, 0.0, (32, 333)).astype(np.float32)
    return np.concatenate([n, u])


def set_c():
    """V = 65 024, 4 rows uniform over [-120, 0]: the terms go denormal, and 0 below -103.97"""
    return np.random.default_rng(120).uniform(-120.0, 0.0, (4, V_MODEL)).astype(np.float32)


def set_d(V=V_ODD):
    """edge rows: the maximum at index 0, at V-1, a row with -inf entries (one of them at index 0, the scan's start), a plain row"""
    x = (np.random.default_rng(4).standard_normal((4, V)) * 8.0).astype(np.float32)
    x[0, 0] = x[0].max() + 1.0
    x[1, V - 1] = x[1].max() + 1.0
    x[2, ::7] = -np.inf
    if V > 1:
        x[2, 1] = 3.0
    else:
        x[2, 0] = 3.0
    return x


def targets_for(rows, seed, shift=0):
    """one target per row, cycling through: 0, V-1, the argmax, a random id (shift: where row 0 starts in that cycle)"""
    R, V = rows.shape
    rng = np.random.default_rng(seed)
    kinds = [np.zeros(R, np.int64), np.full(R, V - 1), rows.argmax(axis=1), rng.integers(0, V, R)]
    return np.array([kinds[(r + shift) % 4][r] for r in range(R)], np.int32)


def reversed_sum(terms):
    """the row's double sum taken from the last element to the first (np.cumsum is one sequential chain)"""
    return float(np.cumsum(terms[::-1].astype(np.float64))[-1])


def strided_sum(terms, lanes=64):
    """64 lanes, lane i summing elements i, i + 64, ... in order, then the lanes in order"""
    t = np.zeros((terms.size + lanes - 1) // lanes * lanes, np.float64)
    t[:terms.size] = terms
    return float(np.cumsum(np.cumsum(t.reshape(-1, lanes), axis=0)[-1])[-1])
