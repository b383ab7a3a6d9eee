"""Shared by tests/test_logprob_cpu.py and tests/test_gpu_logprob.py: the host harness (tests/host/logprob_harness.cpp, built with
g++ like score_ref.build_harness), the numpy yardstick of the top-n order, and the tie set."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V_TIES = 4000


def build_harness(tmp_dir):
    so = os.path.join(str(tmp_dir), "liblogprob_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I",
                           os.path.join(ROOT, "ggllm.cpp_amd", "csrc"), "-o", so, os.path.join(ROOT, "tests", "host", "logprob_harness.cpp")])
    H = C.CDLL(so)
    H.logprob_fq.restype = None
    H.logprob_fq.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 5
    return H


def host_logprob(H, rows, chosen, n_top, V=None):
    """rows [R][stride >= V]; returns prob f32 [R], top_id i32 [R][n_top], top_prob f32 [R][n_top], max f32 [R], sum f64 [R]"""
    rows = np.ascontiguousarray(rows, np.float32)
    R, S = rows.shape
    V = S if V is None else V
    ch = np.ascontiguousarray(chosen, np.int32)
    assert ch.shape == (R,) and int(ch.max(initial=-1)) < V and 0 <= n_top <= V
    prob, mx, sm = np.zeros(R, np.float32), np.zeros(R, np.float32), np.zeros(R, np.float64)
    ids, tp = np.zeros((R, n_top), np.int32), np.zeros((R, n_top), np.float32)
    H.logprob_fq(rows.ctypes.data, S, R, V, ch.ctypes.data, n_top, prob.ctypes.data, ids.ctypes.data if n_top else None,
                 tp.ctypes.data if n_top else None, mx.ctypes.data, sm.ctypes.data)
    return prob, ids, tp, mx, sm


def fkey(x):
    """fq_fkey (csrc/fq_sample.h) restated: the float's bits as an unsigned integer whose order is the values' order, -0 below +0"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def top_ids(row, n_top, ties_id_descending=False):
    """the yardstick: ids sorted by the bit key descending, then id ascending (ties_id_descending: the WRONG tie rule, to show the
    comparison can tell them apart). No float comparison."""
    k = fkey(row).astype(np.int64)
    ids = np.arange(row.size, dtype=np.int64)
    order = np.lexsort((-ids if ties_id_descending else ids, -k))            # (last key is the primary one)
    return order[:n_top].astype(np.int32)


def tie_rows(n=8, V=V_TIES, seed=7):
    """the sampler tests' tie rows: small integers, so the maximum is held by hundreds of ids"""
    return np.random.default_rng(seed).integers(-3, 4, (n, V)).astype(np.float32)


def zero_row(V=64):
    """+0.0 and -0.0 lead the row (everything else negative), the -0.0 entries at LOWER ids than the +0.0 ones"""
    x = -1.0 - np.random.default_rng(11).random(V).astype(np.float32)
    x[[3, 9]] = -0.0
    x[[17, 40]] = 0.0
    return x
