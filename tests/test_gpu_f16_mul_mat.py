"""GPU: ggml_hip_mul_mat_f16 (csrc/kernels_f16.hip) against the yardstick of tests/f16_ref.py, bit for bit (uint32): the reference's
scalar ggml_compute_forward_mul_mat_f16_f32 -- columns rounded to fp16, one f64 sum per output, element 0 first.

Shapes: K = 32 (one partial tile), 96 (a 96-element tail), 256 (two whole tiles), 4544 (35 tiles and a 64-element tail), 18176; M = 1, 65 (two row tiles, one
lane in the second), 200; N = 1 (the decode form), 2 and 4 (the lock-step forms), 5 (8-column form, masked), 17 (two groups of 8 and a single), 33, 130
(16 groups and a pair). Both generators in every form at K = 96 and K = 4544."""
import numpy as np
import pytest

import ggllm_cpp_amd as g
import f16_ref

pytestmark = pytest.mark.gpu

NS = (1, 2, 4, 5, 17, 33, 130)
CASES = [(gen, K, 65, N) for gen in f16_ref.GENERATORS for K in (96, 4544) for N in NS]
CASES += [(gen, 32, 1, 1) for gen in f16_ref.GENERATORS] + [(gen, 32, 200, 5) for gen in f16_ref.GENERATORS]
CASES += [(gen, 256, 200, N) for gen in f16_ref.GENERATORS for N in (4, 17)]
CASES += [(gen, 4544, 1, 2) for gen in f16_ref.GENERATORS] + [(gen, 4544, 200, 3) for gen in f16_ref.GENERATORS]
CASES += [(gen, 18176, 200, 1) for gen in f16_ref.GENERATORS] + [(gen, 18176, 65, 5) for gen in f16_ref.GENERATORS]


@pytest.fixture(scope="module", autouse=True)
def _init():
    g.init(0)
    yield
    g.load().ggml_hip_reference_order(0)


def run(w, x, ldx=None):
    W = g.Weight.upload(g.F16, w)
    try:
        assert W.nbytes() == 2 * w.shape[0] * w.shape[1]
        return W.mul_mat_f16(x, ldx)
    finally:
        W.free()


def differing(got, want):
    return int(np.count_nonzero(f16_ref.bits(got) != f16_ref.bits(want)))


@pytest.mark.parametrize("gen,K,M,N", CASES)
def test_bits_equal_the_yardstick(gen, K, M, N):
    w, x, y = f16_ref.case(gen, K, M, N)
    got = run(w, x)
    assert got.shape == y.shape
    assert differing(got, y) == 0, f"{differing(got, y)} of {y.size} outputs differ"


@pytest.mark.parametrize("gen", list(f16_ref.GENERATORS))
@pytest.mark.parametrize("K,M,N,ldx", [(96, 65, 5, 100), (4544, 65, 2, 4544 + 37), (4544, 65, 17, 2 * 4544), (256, 200, 1, 257)])
def test_rows_of_x_further_apart_than_k(gen, K, M, N, ldx):
    w, x, y = f16_ref.case(gen, K, M, N)
    assert differing(run(w, x, ldx), y) == 0


@pytest.mark.parametrize("gen", list(f16_ref.GENERATORS))
@pytest.mark.parametrize("K", [96, 4544])
def test_a_tokens_bits_do_not_depend_on_n(gen, K):
    w, x, y = f16_ref.case(gen, K, 65, 130)
    W = g.Weight.upload(g.F16, w)
    try:
        whole = W.mul_mat_f16(x)
        for t in (0, 1, 7, 8, 127, 128, 129):                     # first / last column of a group, the group of two at the end
            for n in (1, 2, 4, 5):                                 # the token as the LAST column of every narrower form
                lo = max(0, t - n + 1)
                part = W.mul_mat_f16(x[lo:t + 1])
                assert np.array_equal(f16_ref.bits(part[-1]), f16_ref.bits(whole[t])), (t, n)
        assert differing(whole, y) == 0
    finally:
        W.free()


@pytest.mark.parametrize("gen", list(f16_ref.GENERATORS))
def test_reference_order_does_not_change_the_bits(gen):
    L = g.load()
    w, x, y = f16_ref.case(gen, 4544, 65, 5)
    W = g.Weight.upload(g.F16, w)
    try:
        for mode in (0, 1, 2):
            L.ggml_hip_reference_order(mode)
            for n in (1, 2, 5):
                assert differing(W.mul_mat_f16(x[:n]), y[:n]) == 0, (mode, n)
            assert differing(W.mul_mat(x), y) == 0, mode                 # ggml_hip_mul_mat_q forwards F16 weights
    finally:
        L.ggml_hip_reference_order(0)
        W.free()


def test_get_rows_is_an_exact_widening():
    rng = np.random.default_rng(5)
    K, M = 96, 200
    h = rng.integers(0, 1 << 16, size=(M, K), dtype=np.uint16)
    h[(h & 0x7C00) == 0x7C00] &= 0x83FF                                  # (no inf / nan: every other pattern, subnormals included)
    w = h.view(np.float16)
    W = g.Weight.upload(g.F16, w)
    try:
        assert np.array_equal(f16_ref.bits(W.dequantize()), f16_ref.bits(w.astype(np.float32)))
        rows = [199, 0, 64, 63, 0, 130]
        assert np.array_equal(f16_ref.bits(W.dequantize(rows)), f16_ref.bits(w[rows].astype(np.float32)))
    finally:
        W.free()
