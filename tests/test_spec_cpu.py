"""CPU: the draft rules of draft-and-verify decode. tests/spec_ref.py restates them; ggllm.cpp_amd/csrc/fq_spec.h, what the device
compiles, is host-compiled with g++ (tests/host/spec_harness.cpp) and must agree -- both of its forms of the lookup: the rule as it
reads and the one max-reduction over suffix keys the kernel runs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import spec_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LOOKUP_CASES = sr.LOOKUP_CASES


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("spec") / "libspec_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I", os.path.join(ROOT, "ggllm.cpp_amd", "csrc"),
                           "-o", out, os.path.join(ROOT, "tests", "host", "spec_harness.cpp")])
    L = C.CDLL(out)
    vp = C.c_void_p
    L.spec_lookup_seq.restype, L.spec_lookup_seq.argtypes = C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    L.spec_lookup_keys.restype, L.spec_lookup_keys.argtypes = None, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    L.spec_given_draft.restype, L.spec_given_draft.argtypes = C.c_int, [vp, C.c_int, C.c_int, C.c_int]
    L.spec_simulate.restype = C.c_int
    L.spec_simulate.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp]
    assert L.spec_state_words() == 7 + 16
    return L


def host_lookup(H, fn, h, gmin, gmax, K):
    a = np.ascontiguousarray(list(h) + [0], np.int32)           # (never empty)
    d = np.full(K, -7, np.int32)
    fn(a.ctypes.data, len(h), gmin, gmax, K, d.ctypes.data)
    return d.tolist()


def host_simulate(H, truth, K, source, history=(), ngram=(1, 3), guess=(), pos=0, n_ctx=0):
    t = np.ascontiguousarray(truth, np.int32)
    h = np.zeros(len(history) + len(truth) + 1, np.int32)
    h[:len(history)] = history
    q = np.ascontiguousarray(list(guess) + [0], np.int32)
    per = np.zeros(len(truth) + 1, np.int32)
    n = H.spec_simulate(t.ctypes.data, t.size, K, source, h.ctypes.data, len(history), ngram[0], ngram[1], q.ctypes.data, len(guess), pos, n_ctx, per.ctypes.data)
    assert h[:len(history) + len(truth)].tolist() == list(history) + list(truth)
    return per[:n].tolist()


@pytest.mark.parametrize("name,h,gmin,gmax,K,want", LOOKUP_CASES, ids=[c[0] for c in LOOKUP_CASES])
def test_lookup_rule_by_hand(H, name, h, gmin, gmax, K, want):
    assert sr.lookup(h, gmin, gmax, K) == want
    assert host_lookup(H, H.spec_lookup_seq, h, gmin, gmax, K) == want
    assert host_lookup(H, H.spec_lookup_keys, h, gmin, gmax, K) == want


def test_lookup_on_random_histories_all_three_statements_agree(H):
    """an alphabet of 4 makes matches of every length abound"""
    rng = np.random.default_rng(5)
    for _ in range(400):
        n = int(rng.integers(0, 65))
        h = rng.integers(0, 4, n).tolist()
        gmin = int(rng.integers(1, 4))
        gmax = gmin + int(rng.integers(0, 4))
        K = int(rng.integers(1, 16))
        want = sr.lookup(h, gmin, gmax, K)
        assert host_lookup(H, H.spec_lookup_seq, h, gmin, gmax, K) == want
        assert host_lookup(H, H.spec_lookup_keys, h, gmin, gmax, K) == want


def test_given_alignment(H):
    q = [10, 11, 12, 13, 14]
    assert sr.given(q, 0, 3) == [10, 11, 12]             # q[i] guesses draw i; row 0 holds the pending token, which nobody guesses
    assert sr.given(q, 3, 3) == [13, 14, -1]
    assert sr.given(q, 7, 2) == [-1, -1]
    a = np.ascontiguousarray(q, np.int32)
    for s in range(8):
        assert [H.spec_given_draft(a.ctypes.data, len(q), s, i) for i in (1, 2, 3)] == sr.given(q, s, 3)


def test_given_passes_accept_all_some_none(H):
    truth = list(range(100, 124))
    for K in (1, 3, 7, 15):
        per, hist = sr.simulate(truth, K, sr.GIVEN, guess=truth)
        assert len(per) == -(-24 // (K + 1)) and sum(per) == 24 and all(d == K + 1 for d in per[:-1])
        assert host_simulate(H, truth, K, sr.GIVEN, guess=truth) == per
        wrong = [t + 1000 for t in truth]
        per, hist = sr.simulate(truth, K, sr.GIVEN, guess=wrong)
        assert per == [1] * 24 and hist == [24] + [0] * K
        assert host_simulate(H, truth, K, sr.GIVEN, guess=wrong) == per
    bad = list(truth)
    bad[5] += 1000
    bad[6] += 1000
    per, hist = sr.simulate(truth, 3, sr.GIVEN, guess=bad)
    # draws 0-3 | 4 and 5 (the guess of 5 is wrong: the pass stops behind it) | 6 (guessed wrong) | 7-10 | 11-14 | 15-18 | 19-22 | 23
    assert per == [4, 2, 1, 4, 4, 4, 4, 1] and hist == [2, 1, 0, 5]
    assert host_simulate(H, truth, 3, sr.GIVEN, guess=bad) == per


def test_lookup_passes_on_a_repetitive_text(H):
    period = [3, 1, 4, 1, 5, 9, 2, 6]
    history = period * 2 + period[:3]
    truth = (period * 6)[3:3 + 30]
    per, hist = sr.simulate(truth, 3, sr.LOOKUP, history=history, ngram=(1, 3))
    assert per == [4] * 7 + [2] and hist == [0, 1, 0, 7]              # every draft right: ceil(30 / 4) passes
    assert host_simulate(H, truth, 3, sr.LOOKUP, history=history, ngram=(1, 3)) == per
    rng = np.random.default_rng(9)
    for _ in range(100):
        history = rng.integers(0, 4, int(rng.integers(1, 20))).tolist()
        truth = rng.integers(0, 4, int(rng.integers(1, 40))).tolist()
        K = int(rng.integers(1, 16))
        per, hist = sr.simulate(truth, K, sr.LOOKUP, history=history, ngram=(1, 3))
        assert sum(per) == len(truth) and sum(hist) == len(per)
        assert host_simulate(H, truth, K, sr.LOOKUP, history=history, ngram=(1, 3)) == per


def test_no_row_at_or_past_the_end_of_the_cache_is_accepted(H):
    """pending token at position 20 of a cache of 32, K = 7, every draft right: the draw made at position 31 is the last one a
    pass may make (its successor would sit at 32), so the run of 12 draws is 8 + 4, not 8 + 4 with a fifth row looked at"""
    truth = list(range(50, 62))
    per, hist = sr.simulate(truth, 7, sr.GIVEN, guess=truth + [99, 98, 97], pos=20, n_ctx=32)
    assert per == [8, 4]
    assert host_simulate(H, truth, 7, sr.GIVEN, guess=truth + [99, 98, 97], pos=20, n_ctx=32) == per
    per, _ = sr.simulate(truth[:11], 7, sr.GIVEN, guess=truth, pos=21, n_ctx=32)
    assert per == [8, 3]
