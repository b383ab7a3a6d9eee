"""The yardstick of the F16 mat-mul (ggml_compute_forward_mul_mat_f16_f32 over the scalar ggml_vec_dot_f16) in numpy, and the two
input generators its tests share.

Contract (csrc/fq_f16.h): the activation column is rounded to fp16; sum is a DOUBLE that starts at 0 and takes
(double)((float) w[r][i] * (float) x16[n][i]) for i = 0 .. K-1 in that order; dst = (float) sum. The f32 product of two fp16 values is
exact, so the f64 product below is the same number; np.add.accumulate is strictly sequential (np.sum is pairwise, it is not)."""
import functools

import numpy as np


def yardstick(w16, x):
    """w16 [M, K] float16, x [N, K] float32 -> [N, M] float32"""
    w16 = np.asarray(w16, np.float16)
    x = np.asarray(x, np.float32).reshape(-1, w16.shape[1])
    w64 = w16.astype(np.float64)
    x16 = x.astype(np.float16)
    out = np.empty((x.shape[0], w16.shape[0]), np.float32)
    for n in range(x.shape[0]):
        out[n] = np.add.accumulate(w64 * x16[n].astype(np.float64), axis=1)[:, -1].astype(np.float32)
    return out


def terms(w16, x_row):
    """the f64 terms of every row for one token: [M, K]"""
    return np.asarray(w16, np.float16).astype(np.float64) * np.asarray(x_row, np.float32).astype(np.float16).astype(np.float64)


# other associations of the same terms (what a parallel kernel would do), each -> [M] float32
def order_sequential(t):
    return np.add.accumulate(t, axis=1)[:, -1].astype(np.float32)


def order_reversed(t):
    return np.add.accumulate(t[:, ::-1], axis=1)[:, -1].astype(np.float32)


def order_groups_of_8(t):
    M, K = t.shape
    g = np.add.accumulate(t.reshape(M, K // 8, 8), axis=2)[:, :, -1]
    return np.add.accumulate(g, axis=1)[:, -1].astype(np.float32)


def order_strided_lanes(t, lanes=64):
    M, K = t.shape
    pad = (-K) % lanes
    tp = np.concatenate([t, np.zeros((M, pad))], axis=1).reshape(M, -1, lanes)      # [M, steps, lane]: lane l takes terms l, l + 64, ...
    part = np.add.accumulate(tp, axis=1)[:, -1, :]
    return np.add.accumulate(part, axis=1)[:, -1].astype(np.float32)


EDGE = np.array([1e-5, -3e-6, 6.1e-5, 5.96e-8, 2.9e-8, 0.0, 1.00048828125, 65504.0], np.float32)      # subnormal results, a rounding tie, the largest fp16


def model_like(K, M, N, seed=0):
    """weights N(0, 0.02^2) as fp16, activations N(0, 1) as f32; token 0 starts with EDGE"""
    rng = np.random.default_rng(1000 + seed)
    w = (rng.standard_normal((M, K)) * 0.02).astype(np.float32).astype(np.float16)
    x = rng.standard_normal((N, K)).astype(np.float32)
    x[0, :EDGE.size] = EDGE
    return w, x


def cancelling_rows(K, M, N, seed=0):
    """rows built so that the ORDER of the sum decides the f32 result: tiny terms everywhere, and four huge ones (x = 32768 against
    weights +b, -b, +b', -b') that cancel exactly"""
    rng = np.random.default_rng(2000 + seed)

    def pm(shape):
        return rng.integers(0, 2, size=shape) * 2.0 - 1.0

    x = (pm((N, K)) * 2.0 ** rng.uniform(-15, -13, size=(N, K))).astype(np.float32)
    w = (pm((M, K)) * 2.0 ** rng.uniform(-15, -11, size=(M, K))).astype(np.float32).astype(np.float16)
    pos = np.sort(rng.choice(K, size=4, replace=False))
    x[:, pos] = 32768.0
    b = (pm((M, 2)) * 16.0 * rng.integers(1024, 2048, size=(M, 2))).astype(np.float16)
    w[:, pos[0]], w[:, pos[1]], w[:, pos[2]], w[:, pos[3]] = b[:, 0], -b[:, 0], b[:, 1], -b[:, 1]
    return w, x


GENERATORS = {"model_like": model_like, "cancelling_rows": cancelling_rows}


@functools.lru_cache(maxsize=None)
def case(gen, K, M, N):
    """(w16, x, yardstick), computed once per shape and shared (read-only)"""
    w, x = GENERATORS[gen](K, M, N)
    y = yardstick(w, x)
    for a in (w, x, y):
        a.setflags(write=False)
    return w, x, y


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
