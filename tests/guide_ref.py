"""Shared by tests/test_guide_cpu.py and the GPU guidance tests: the host harness (tests/host/guide_harness.cpp over
csrc/fq_guide.h, built with g++) and an independent numpy restatement of the pinned summation order and the mix."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES, GROUP = 256, 4


def build_harness(tmp_dir):
    so = os.path.join(str(tmp_dir), "libguide_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I",
                           os.path.join(ROOT, "ggllm.cpp_amd", "csrc"), "-o", so, os.path.join(ROOT, "tests", "host", "guide_harness.cpp")])
    H = C.CDLL(so)
    H.guide_rows.restype = None
    H.guide_rows.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    for f in (H.guide_expf, H.guide_logf):
        f.restype, f.argtypes = None, [C.c_void_p, C.c_void_p, C.c_int64]
    return H


def host_mix(H, rows, V, lead, guide, scale, fill=np.nan):
    """H.guide_rows over rows [R][stride >= V]: mixed [P][V], max [P][2] f32, sum [P][2] f64; a skipped pair (lead < 0) keeps `fill`"""
    rows = np.ascontiguousarray(rows, np.float32)
    lead, guide = np.ascontiguousarray(lead, np.int32), np.ascontiguousarray(guide, np.int32)
    scale = np.ascontiguousarray(scale, np.float32)
    P = lead.size
    assert guide.size == P and scale.size == P and int(max(lead.max(), guide.max())) < rows.shape[0]
    mixed, mx, sm = np.full((P, V), fill, np.float32), np.full((P, 2), fill, np.float32), np.full((P, 2), fill, np.float64)
    H.guide_rows(rows.ctypes.data, rows.shape[1], V, P, lead.ctypes.data, guide.ctypes.data, scale.ctypes.data, mixed.ctypes.data, V,
                 mx.ctypes.data, sm.ctypes.data)
    return mixed, mx, sm


def _libm(fn, x):
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(x)
    fn(x.ctypes.data, out.ctypes.data, x.size)
    return out


def terms(H, x):
    """the row's maximum and its float terms expf(x - max)"""
    x = np.asarray(x, np.float32)
    m = x.max()
    return m, _libm(H.guide_expf, x - m)


def pinned_sum(e):
    """the double sum of the float terms e in the pinned order: 256 partial sums, element v to sum (v // 4) % 256, each in increasing v
    (np.cumsum is one sequential chain), then q_j += q_{j xor o} for o = 1, 2, .., 128; q_0"""
    n = e.size
    per = LANES * GROUP
    t = np.zeros((n + per - 1) // per * per, np.float64)      # (adding +0.0 to a partial sum >= 0 changes no bit)
    t[:n] = e
    lanes = t.reshape(-1, LANES, GROUP).transpose(1, 0, 2).reshape(LANES, -1)      # lane j: its elements in increasing v
    q = np.cumsum(lanes, axis=1)[:, -1]
    j = np.arange(LANES)
    o = 1
    while o < LANES:
        q = q + q[j ^ o]
        o *= 2
    return float(q[0])


def index_order_sum(e):
    """the same terms summed in index order (ggml_hip_score_rows' chain)"""
    return float(np.cumsum(e.astype(np.float64))[-1])


def numpy_pair(H, xb, xg, scale):
    """the issue's arithmetic restated with numpy float32 / float64 operations; the two libm calls are the harness's: y f32 [V], (max_b, max_g), (S_b, S_g)"""
    lp, ms, Ss = [], [], []
    for x in (np.asarray(xb, np.float32), np.asarray(xg, np.float32)):
        m, e = terms(H, x)
        S = pinned_sum(e)
        L = _libm(H.guide_logf, np.array([S], np.float64).astype(np.float32))[0]
        lp.append((x - m) - L)
        ms.append(m)
        Ss.append(S)
    d = lp[0] - lp[1]
    p = np.float32(scale) * d
    return (lp[1] + p).astype(np.float32), ms, Ss
