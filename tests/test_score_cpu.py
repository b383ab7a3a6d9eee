"""CPU: the scoring arithmetic the device compiles (ggllm.cpp_amd/csrc/fq_score.h) against the reference's own three lines
with the host libm's expf (tests/host/score_harness.cpp: score_fq / score_libm), bit for bit -- and the yardstick check: on
the rows these tests use, a double sum taken in another order (reversed, 64 strided lanes) does NOT give the sequential
sum's bits, so comparing the 64 bits of `sum` catches a kernel that re-associates it (the rounded float prob would not)."""
import numpy as np
import pytest

import score_ref as sr


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return sr.build_harness(tmp_path_factory.mktemp("score"))


def _same(H, rows, seed):
    """score_fq == score_libm with each of the four target kinds (0, V-1, argmax, random) on every row"""
    R = rows.shape[0]
    for shift in range(4):
        tg = sr.targets_for(rows, seed + shift, shift)
        a, b = sr.host_score(H.score_fq, rows, tg), sr.host_score(H.score_libm, rows, tg)
        assert np.array_equal(a[1], b[1]), "max"
        assert np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64)), "sum bits"
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), "prob bits"
        assert np.all(np.isfinite(a[0])) and np.all(a[0] >= 0) and np.all(a[0] <= 1) and R == a[0].size


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "d1"])
def test_fq_score_equals_the_reference_lines_with_libm(H, name):
    rows = {"a": sr.set_a, "b": sr.set_b, "c": sr.set_c, "d": sr.set_d, "d1": lambda: sr.set_d(1)}[name]()
    _same(H, rows, 7)


def test_terms_of_the_wide_rows_go_denormal_and_zero(H):
    """set (c) is what it claims: denormal terms, and exact zeros below -103.97"""
    rows = sr.set_c()
    _, mx, _, terms = sr.host_score(H.score_fq, rows, np.zeros(4, np.int32), want_terms=True)
    tiny = np.finfo(np.float32).tiny
    assert ((terms > 0) & (terms < tiny)).sum() > 1000 and (terms == 0).sum() > 1000
    assert np.all(terms[(rows - mx[:, None]) < -103.98] == 0)


@pytest.mark.parametrize("name", ["a", "b_normal", "b_uniform"])
def test_other_orders_move_the_sum(H, name):
    """the yardstick: reversed and 64-strided double sums each differ from the sequential one in at least half of the rows
    (these seeds: 16/16 and 16/16 at V = 65 024; at V = 333 31/32 and 30/32 of the normal rows, 28/32 and 29/32 of the uniform ones)"""
    rows = {"a": sr.set_a, "b_normal": lambda: sr.set_b()[:32], "b_uniform": lambda: sr.set_b()[32:]}[name]()
    R = rows.shape[0]
    _, _, sm, terms = sr.host_score(H.score_fq, rows, np.zeros(R, np.int32), want_terms=True)
    seq = np.array([float(np.cumsum(t.astype(np.float64))[-1]) for t in terms])
    assert np.array_equal(seq.view(np.uint64), sm.view(np.uint64))          # (np.cumsum IS the sequential chain)
    rev = np.array([sr.reversed_sum(t) for t in terms])
    stri = np.array([sr.strided_sum(t) for t in terms])
    n_rev, n_str = int((rev != sm).sum()), int((stri != sm).sum())
    print(f"{name}: reversed differs in {n_rev}/{R} rows, 64-strided in {n_str}/{R}")
    assert 2 * n_rev >= R and 2 * n_str >= R
