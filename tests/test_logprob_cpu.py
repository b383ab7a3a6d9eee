"""CPU: the log-probability record the device compiles (ggllm.cpp_amd/csrc/fq_logprob.h through tests/host/logprob_harness.cpp)
against the scoring harness (score_fq: max, the sum's 64 bits, every probability's 32 bits) and against a numpy yardstick of the
top-n order built from the floats' bits."""
import numpy as np
import pytest

import logprob_ref as lr
import score_ref as sr

N_TOPS = [1, 5, 32]


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return lr.build_harness(tmp_path_factory.mktemp("logprob"))


@pytest.fixture(scope="module")
def HS(tmp_path_factory):
    return sr.build_harness(tmp_path_factory.mktemp("score"))


def _rows(name):
    return {"a": sr.set_a, "b": sr.set_b, "c": sr.set_c, "d": sr.set_d, "d1": lambda: sr.set_d(1)}[name]()


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "d1"])
def test_record_equals_score_fq(H, HS, name):
    """max, the sum's 64 bits and the chosen probability's 32 bits are score_fq's; every listed top id's probability is score_fq's
    with that id as target; the ids are the yardstick's"""
    rows = _rows(name)
    R, V = rows.shape
    ch = sr.targets_for(rows, 21)
    want_p, want_m, want_s = sr.host_score(HS.score_fq, rows, ch)
    for n_top in [n for n in N_TOPS if n <= V]:
        p, ids, tp, mx, sm = lr.host_logprob(H, rows, ch, n_top)
        assert np.array_equal(mx, want_m), "max"
        assert np.array_equal(sm.view(np.uint64), want_s.view(np.uint64)), "sum bits"
        assert np.array_equal(p.view(np.uint32), want_p.view(np.uint32)), "prob bits"
        assert np.array_equal(ids, np.stack([lr.top_ids(r, n_top) for r in rows])), "top ids"
        for j in range(n_top):
            pj = sr.host_score(HS.score_fq, rows, ids[:, j])[0]
            assert np.array_equal(tp[:, j].view(np.uint32), pj.view(np.uint32)), f"top prob {j}"
        assert np.all(np.diff(tp.astype(np.float64), axis=1) <= 0)


def test_negative_chosen_is_nan_and_keeps_the_top(H):
    rows = sr.set_b()[:4]
    ch = np.array([-1, 5, -1, 0], np.int32)
    p, ids, tp, _, _ = lr.host_logprob(H, rows, ch, 5)
    q, ids2, tp2, _, _ = lr.host_logprob(H, rows, np.array([7, 5, 7, 0], np.int32), 5)
    assert np.isnan(p[[0, 2]]).all() and np.array_equal(p[[1, 3]].view(np.uint32), q[[1, 3]].view(np.uint32))
    assert np.array_equal(ids, ids2) and np.array_equal(tp.view(np.uint32), tp2.view(np.uint32))


def test_minus_inf_entries_rank_last_with_probability_zero(H):
    """set d's -inf row at V = 33: 28 finite entries, n_top 32 lists them first, then -inf ids in ascending order with probability 0"""
    rows = sr.set_d(33)[2:3]
    finite = int(np.isfinite(rows[0]).sum())
    assert finite < 32
    _, ids, tp, _, _ = lr.host_logprob(H, rows, np.zeros(1, np.int32), 32)
    assert np.array_equal(ids[0], lr.top_ids(rows[0], 32))
    assert np.all(np.isfinite(rows[0][ids[0, :finite]])) and np.all(np.isneginf(rows[0][ids[0, finite:]]))
    assert np.all(np.diff(ids[0, finite:]) > 0) and np.all(tp[0, finite:] == 0) and np.all(tp[0, :finite] > 0)


@pytest.mark.parametrize("n_top", N_TOPS)
def test_tie_set(H, n_top):
    """ties: the ids are the lowest ids holding the maximum; the wrong tie rule (id descending) gives another list in EVERY row, so a
    comparison of ids catches it"""
    rows = lr.tie_rows()
    _, ids, _, _, _ = lr.host_logprob(H, rows, np.zeros(rows.shape[0], np.int32), n_top)
    for r, row in enumerate(rows):
        assert np.array_equal(ids[r], np.flatnonzero(row == row.max())[:n_top])
        assert np.array_equal(ids[r], lr.top_ids(row, n_top))
        assert not np.array_equal(ids[r], lr.top_ids(row, n_top, ties_id_descending=True))


def test_positive_zero_ranks_above_negative_zero(H):
    row = lr.zero_row()
    _, ids, tp, _, _ = lr.host_logprob(H, row[None, :], np.zeros(1, np.int32), 5)
    assert ids[0, :4].tolist() == [17, 40, 3, 9]
    assert np.array_equal(ids[0], lr.top_ids(row, 5))
    assert len(set(tp[0, :4].view(np.uint32).tolist())) == 1           # (the same value, the same probability)
