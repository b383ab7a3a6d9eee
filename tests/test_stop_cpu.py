"""CPU: the stop rule the device sampler compiles (ggllm.cpp_amd/csrc/fq_stop.h) is host-compiled with g++
(tests/host/stop_harness.cpp) and checked against a restatement of the rule in Python: random streams over a small alphabet,
and the edge cases by hand."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ggllm_cpp_amd as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNNING, BUDGET = g.STOP_RUNNING, g.STOP_BUDGET


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("stop") / "libstop_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I", os.path.join(ROOT, "ggllm.cpp_amd", "csrc"),
                           "-o", out, os.path.join(ROOT, "tests", "host", "stop_harness.cpp")])
    L = C.CDLL(out)
    L.stop_reset.argtypes = [C.c_void_p]
    L.stop_draw.restype, L.stop_draw.argtypes = C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    L.stop_run.restype = C.c_int
    L.stop_run.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    assert L.stop_state_words() == 10
    return L


def rule(seqs, max_tokens, drawn):
    """THE rule, restated: the reason after the last token of `drawn` (every token drawn since the stops were set)"""
    n = len(drawn)
    for k, q in enumerate(seqs):
        if len(q) <= n and list(drawn[n - len(q):]) == list(q):
            return k
    if max_tokens > 0 and n == max_tokens:
        return BUDGET
    return RUNNING


class Row:
    """one row of fq_stop.h on the host"""

    def __init__(self, H, seqs, max_tokens=0):
        self.H, self.max_tokens, self.n = H, max_tokens, len(seqs)
        self.len = np.zeros(16, np.int32)
        self.tok = np.zeros((16, 8), np.int32)
        for k, q in enumerate(seqs):
            self.len[k] = len(q)
            self.tok[k, :len(q)] = q
        self.state = np.zeros(10, np.int32)
        self.reset()

    def reset(self):
        self.H.stop_reset(self.state.ctypes.data)

    def draw(self, t):
        return self.H.stop_draw(self.n, self.len.ctypes.data, self.tok.ctypes.data, self.max_tokens, self.state.ctypes.data, int(t))

    def run(self, stream):
        s = np.ascontiguousarray(stream, np.int32)
        out = np.zeros(max(s.size, 1), np.int32)
        n = self.H.stop_run(self.n, self.len.ctypes.data, self.tok.ctypes.data, self.max_tokens, self.state.ctypes.data, s.ctypes.data, s.size, out.ctypes.data)
        return out[:n].tolist()


def test_random_streams_match_the_restated_rule(H):
    """a 6-token alphabet makes sequences of every length complete often; after each end the stops are set again, as a caller would"""
    rng = np.random.default_rng(20)
    draws = ends = 0
    for trial in range(300):
        seqs = [rng.integers(0, 6, int(rng.integers(1, 9))).tolist() for _ in range(int(rng.integers(0, 17)))]
        if trial % 3 == 0:
            seqs = [q for q in seqs if len(q) >= 3]          # (without short sequences the long ones get their turn)
        max_tokens = int(rng.integers(0, 40)) if trial % 2 else 0
        row, drawn = Row(H, seqs, max_tokens), []
        for t in rng.integers(0, 6, 24).tolist():
            drawn.append(t)
            want = rule(seqs, max_tokens, drawn)
            assert row.draw(t) == want, (seqs, max_tokens, drawn)
            assert row.state[0] == len(drawn) and row.state[1] == want
            draws += 1
            if want != RUNNING:
                row.reset()
                drawn = []
                ends += 1
    assert draws >= 5000 and ends >= 500


def test_overlapping_sequences(H):
    """[1, 1, 2] in 1 1 1 2: the match is found although an earlier attempt at it failed one token in"""
    assert Row(H, [[1, 1, 2]]).run([1, 1, 1, 2, 5]) == [RUNNING, RUNNING, RUNNING, 0]
    assert Row(H, [[1, 2, 1, 2, 3]]).run([1, 2, 1, 2, 1, 2, 3]) == [RUNNING] * 6 + [0]
    # a sequence that is the tail of another: both complete at the same draw when the longer does
    assert Row(H, [[4, 5, 3], [5, 3]]).run([4, 5, 3]) == [RUNNING, RUNNING, 0]
    assert Row(H, [[4, 5, 3], [5, 3]]).run([0, 5, 3]) == [RUNNING, RUNNING, 1]


def test_lowest_index_wins_when_two_complete_at_one_draw(H):
    assert Row(H, [[9], [2, 3], [3]]).run([2, 3]) == [RUNNING, 1]
    assert Row(H, [[9], [3], [2, 3]]).run([2, 3]) == [RUNNING, 1]
    assert Row(H, [[3], [3]]).run([3]) == [0]


def test_sequence_longer_than_the_draws_cannot_match(H):
    """the fresh tail holds no token: a sequence is not matched by what the tail starts with, nor by fewer draws than it has tokens"""
    for tok in (0, 5):
        assert Row(H, [[tok, tok, tok]]).run([tok, tok]) == [RUNNING, RUNNING]
    eight = [1, 2, 3, 4, 5, 0, 1, 2]
    assert Row(H, [eight]).run(eight[1:] + eight) == [RUNNING] * 14 + [0]
    assert Row(H, [eight]).run(eight) == [RUNNING] * 7 + [0]


def test_sequence_across_a_reset_does_not_match(H):
    row = Row(H, [[2, 3]])
    assert row.draw(2) == RUNNING
    row.reset()                                             # (the stops set again: the 2 is no longer a drawn token)
    assert row.draw(3) == RUNNING and row.state[0] == 1
    assert row.draw(2) == RUNNING and row.draw(3) == 0 and row.state[0] == 3


def test_sequence_wins_over_the_budget_at_the_same_draw(H):
    assert Row(H, [[7, 8]], max_tokens=2).run([7, 8]) == [RUNNING, 0]
    assert Row(H, [[7, 8]], max_tokens=2).run([7, 9]) == [RUNNING, BUDGET]
    assert Row(H, [[7, 8]], max_tokens=3).run([7, 8, 1]) == [RUNNING, 0]


def test_budget_of_one(H):
    assert Row(H, [], max_tokens=1).run([5, 5]) == [BUDGET]
    assert Row(H, [[5]], max_tokens=1).run([5]) == [0]
    assert Row(H, [], max_tokens=0).run([5] * 40) == [RUNNING] * 40


def test_stops_helper_builds_the_structure():
    st = g.stops([[1, 2], [3]], max_tokens=9)
    assert (st.n_seqs, st.max_tokens, list(st.len)[:3], list(st.tok[0])[:2], st.tok[1][0]) == (2, 9, [2, 1, 0], [1, 2], 3)
    assert C.sizeof(g.Stops) == 4 * (1 + 16 + 16 * 8 + 1)
    with pytest.raises(ValueError):
        g.stops([[1]] * 17)
    with pytest.raises(ValueError):
        g.stops([[1] * 9])
    with pytest.raises(ValueError):
        g.stops([[]])
