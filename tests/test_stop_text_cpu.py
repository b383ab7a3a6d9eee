"""CPU: the stop-string rule the device sampler compiles (ggllm.cpp_amd/csrc/fq_stop_text.h behind fq_stop.h) is host-compiled with
g++ (tests/host/stop_text_harness.cpp) and checked against its restatement in Python (tests/stop_text_ref.py: bytes.find over the
growing text): random streams over a three-letter alphabet, and the edge cases by name. Every draw any test makes is also written to
a file of cases, which the same harness -- built as a program of its own with -fsanitize=address,undefined -- replays."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ggllm_cpp_amd as g
import stop_text_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "host", "stop_text_harness.cpp")
GXX = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "ggllm.cpp_amd", "csrc")]
RUNNING, BUDGET, TEXT0 = g.STOP_RUNNING, g.STOP_BUDGET, g.STOP_TEXT0


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("stop_text") / "libstop_text_host.so")
    subprocess.check_call(GXX + ["-O2", "-fPIC", "-shared", "-o", out, HARNESS])
    L = C.CDLL(out)
    vp = C.c_void_p
    L.row_init.argtypes = [vp]
    L.row_set_text.argtypes = [vp, C.c_int, vp, vp]
    L.row_set_ids.argtypes = [vp, C.c_int, vp, vp, C.c_int]
    L.row_draw.restype, L.row_draw.argtypes = C.c_int, [vp, C.c_int, vp, C.c_int, vp]
    L.row_skip_bytes.argtypes = [vp, C.c_int]
    L.row_run.restype, L.row_run.argtypes = C.c_int, [vp, vp, vp, vp, C.c_int, vp]
    L.cases = []                                            # every operation of every test below, for the sanitized replay
    return L


class Row:
    """one row of the harness next to its restatement: every draw is checked, and logged for the replay"""

    def __init__(self, H, vocab):
        self.H, self.vocab, self.want = H, vocab, ref.Restated()
        self.mem = np.zeros(H.row_bytes(), np.uint8)
        H.row_init(self.mem.ctypes.data)
        H.cases.append([0, len(vocab)] + [x for b in vocab for x in [len(b)] + list(b)])
        H.cases.append([1])

    def set_text(self, strings):
        strings = [s if isinstance(s, bytes) else s.encode() for s in strings]
        ln = np.array([len(s) for s in strings] + [0], np.int32)
        by = np.zeros((len(strings) + 1, 32), np.uint8)
        for k, s in enumerate(strings):
            by[k, :len(s)] = list(s)
        self.H.row_set_text(self.mem.ctypes.data, len(strings), ln.ctypes.data, by.ctypes.data)
        self.want.set_text(strings)
        self.H.cases.append([2, len(strings)] + [x for s in strings for x in [len(s)] + list(s)])

    def set_ids(self, seqs, max_tokens=0):
        ln = np.array([len(q) for q in seqs] + [0], np.int32)
        tk = np.zeros((len(seqs) + 1, 8), np.int32)
        for k, q in enumerate(seqs):
            tk[k, :len(q)] = q
        self.H.row_set_ids(self.mem.ctypes.data, len(seqs), ln.ctypes.data, tk.ctypes.data, max_tokens)
        self.want.set_ids(seqs, max_tokens)
        self.H.cases.append([3, len(seqs), max_tokens] + [x for q in seqs for x in [len(q)] + list(q)])

    def skip(self, add):
        self.H.row_skip_bytes(self.mem.ctypes.data, add)
        self.H.cases.append([5, add])

    def draw(self, t):
        """(reason, n_drawn, cut_bytes) after drawing token t -- asserted equal to the restatement's"""
        b = np.frombuffer(self.vocab[t] or b"\0", np.uint8)
        out = np.zeros(3, np.int32)
        self.H.row_draw(self.mem.ctypes.data, int(t), b.ctypes.data, len(self.vocab[t]), out.ctypes.data)
        want = self.want.draw(int(t), self.vocab[t])
        assert tuple(out.tolist()) == want, (t, self.want.strings, self.want.seqs, self.want.ids)
        self.H.cases.append([4, int(t)] + list(want))
        return want

    def run(self, stream):
        """the reasons of a stream of draws, up to and including the one that ends the row"""
        out = []
        for t in stream:
            out.append(self.draw(t))
            if out[-1][0] != RUNNING:
                break
        return out


def vocab_of(*tokens):
    return [t if isinstance(t, bytes) else t.encode() for t in tokens]


def test_random_streams_match_the_restated_rule(H):
    """~50 tokens of a, b, c with lengths 0, 1, 31, 32, 33, 64, 65, 130 and short ones; random strings of 1..32 bytes (short ones complete
    often, long ones are cut from the vocabulary's own long tokens so they can); after each end the strings are set again"""
    rng = np.random.default_rng(31)
    vocab = ref.abc_vocab(rng)
    assert {0, 1, 31, 32, 33, 64, 65, 130} <= {len(b) for b in vocab} and len(vocab) == 50
    draws, ends, long_ends = 0, 0, 0
    for trial in range(160):
        strings = []
        for _ in range(int(rng.integers(1, 17))):
            l = int(rng.integers(1, 33)) if trial % 2 else int(rng.integers(4, 33))
            if rng.random() < 0.5:
                strings.append(bytes(rng.integers(97, 100, l, dtype=np.uint8)))
            else:                                           # a piece of two tokens laid end to end: it can complete
                two = vocab[int(rng.integers(0, 50))] + vocab[int(rng.integers(0, 50))] + b"abc"
                at = int(rng.integers(0, max(1, len(two) - l)))
                strings.append(two[at:at + l])
        row = Row(H, vocab)
        row.set_text(strings)
        if trial % 5 == 0:
            row.set_ids([[int(rng.integers(0, 50))]], max_tokens=int(rng.integers(3, 30)))
        if trial % 7 == 0:
            row.skip((1 << 30) - 64)                        # the byte counter next to its end: it folds, the ring's slots stay
        for t in rng.integers(0, 50, 40).tolist():
            reason, n, cut = row.draw(t)
            draws += 1
            if reason != RUNNING:
                ends += 1
                long_ends += reason >= TEXT0 and len(strings[reason - TEXT0]) >= 8
                row.set_text(strings)
    assert draws >= 3000 and ends >= 300 and long_ends >= 20, (draws, ends, long_ends)


def test_match_spanning_three_tokens(H):
    v = vocab_of("xxHe", "ll", "o!yy", "q")
    assert Row(H, v).run([3, 0, 1, 2]) == [(RUNNING, 1, 0), (RUNNING, 2, 0), (RUNNING, 3, 0), (RUNNING, 4, 0)]
    row = Row(H, v)
    row.set_text(["Hello!"])
    assert row.run([3, 0, 1, 2, 3]) == [(RUNNING, 1, 0), (RUNNING, 2, 0), (RUNNING, 3, 0), (TEXT0, 4, 8)]       # "Hello!yy": 6 + the 2 bytes behind it


def test_match_wholly_inside_a_130_byte_token(H):
    """at its start (a large cut_bytes: the whole token goes), at its end, and past the first 64 bytes; the ring never held these bytes"""
    long = bytes(range(100, 230))
    v = vocab_of(b"ab", long)
    for at, l in ((0, 5), (125, 5), (60, 10), (98, 32), (0, 32)):
        row = Row(H, v)
        row.set_text([long[at:at + l]])
        assert row.run([0, 1, 0]) == [(RUNNING, 1, 0), (TEXT0, 2, 130 - at)]
    row = Row(H, v)                                         # ... and one that starts in the token before
    row.set_text([b"b" + long[:31]])
    assert row.run([0, 1]) == [(RUNNING, 1, 0), (TEXT0, 2, 131)]


def test_two_strings_completing_at_the_same_byte_lowest_k(H):
    v = vocab_of("abcd", "x")
    for strings, k in ((["zz", "bcd", "cd"], 1), (["zz", "cd", "bcd"], 1), (["d", "abcd"], 0), (["xabcd", "d"], 0)):
        row = Row(H, v)
        row.set_text(strings)
        reason, n, cut = row.run([1, 0])[-1]
        assert (reason, n, cut) == (TEXT0 + k, 2, len(strings[k]))


def test_a_higher_k_completing_earlier_in_the_token_wins(H):
    v = vocab_of("abcdef", "x")
    row = Row(H, v)
    row.set_text(["ef", "bc"])
    assert row.run([0]) == [(TEXT0 + 1, 1, 5)]              # "bc" ends at byte 2, "ef" at byte 5
    row.set_text(["xabcdef", "xa"])
    assert row.run([1, 0]) == [(RUNNING, 1, 0), (TEXT0 + 1, 2, 7)]


def test_a_string_longer_than_the_drawn_text_cannot_match(H):
    """a fresh ring holds zeros: a string of zero bytes must not be matched by them, nor a string by fewer bytes than it has"""
    v = vocab_of(b"\0", b"\0\0", "ab", b"")
    row = Row(H, v)
    row.set_text([b"\0\0\0\0"])
    assert row.run([0, 1, 3, 0]) == [(RUNNING, 1, 0), (RUNNING, 2, 0), (RUNNING, 3, 0), (TEXT0, 4, 4)]
    row.set_text(["abab", b"\0ab"])
    assert row.run([2, 3, 2]) == [(RUNNING, 1, 0), (RUNNING, 2, 0), (TEXT0, 3, 4)]      # (a token without bytes matches nothing, and breaks nothing)


def test_id_sequence_and_text_on_the_same_draw_id_wins(H):
    v = vocab_of("ab", "cd")
    row = Row(H, v)
    row.set_text(["bcd"])
    row.set_ids([[9], [0, 1]])
    assert row.run([0, 1]) == [(RUNNING, 1, 0), (1, 2, 0)]
    row.set_ids([[9]])
    assert row.run([0, 1]) == [(RUNNING, 1, 0), (TEXT0, 2, 3)]


def test_text_and_budget_on_the_same_draw_text_wins(H):
    v = vocab_of("ab", "cd")
    row = Row(H, v)
    row.set_text(["bc"])
    row.set_ids([], max_tokens=2)
    assert row.run([0, 1]) == [(RUNNING, 1, 0), (TEXT0, 2, 3)]
    row.set_ids([], max_tokens=2)
    assert row.run([1, 1]) == [(RUNNING, 1, 0), (BUDGET, 2, 0)]


def test_state_split_over_two_calls(H):
    """row_run twice on one state, as two loop calls are: the ring carries the first call's bytes into the second"""
    rng = np.random.default_rng(5)
    vocab = ref.abc_vocab(rng)
    pool, offs = ref.pool_of(vocab)
    stream = np.array([8, 9, 10, 11, 12, 13, 14, 15], np.int32)
    stop = b"".join(vocab[t] for t in stream[:6])[-5:]      # (these tokens have 1..4 bytes: the last 5 bytes of six of them span at least two)
    want, exp = ref.Restated(), []
    want.set_text([stop])
    for t in stream.tolist():
        exp.append(want.draw(t, vocab[t]))
        if exp[-1][0] != RUNNING:
            break
    assert exp[-1][0] == TEXT0 and len(exp) >= 2
    for cut in range(1, len(exp)):
        row = Row(H, vocab)
        row.set_text([stop])
        out = np.zeros((8, 3), np.int32)
        n1 = H.row_run(row.mem.ctypes.data, pool.ctypes.data, offs.ctypes.data, stream.ctypes.data, cut, out.ctypes.data)
        n2 = H.row_run(row.mem.ctypes.data, pool.ctypes.data, offs.ctypes.data, stream[cut:].ctypes.data, 8 - cut, out[cut:].ctypes.data)
        assert n1 == cut and n1 + n2 == len(exp) and [tuple(r) for r in out[:len(exp)].tolist()] == exp
        assert H.row_run(row.mem.ctypes.data, pool.ctypes.data, offs.ctypes.data, stream.ctypes.data, 8, out.ctypes.data) == 0      # (ended: frozen)


def test_reset_by_either_setter(H):
    v = vocab_of("ab", "cd")
    row = Row(H, v)
    row.set_text(["bc"])
    assert row.draw(0) == (RUNNING, 1, 0)
    row.set_text(["bc"])                                    # (the strings set again: the "ab" is no longer drawn text)
    assert row.run([1, 0, 1]) == [(RUNNING, 1, 0), (RUNNING, 2, 0), (TEXT0, 3, 3)]
    row.set_text(["bc"])
    assert row.draw(0) == (RUNNING, 1, 0)
    row.set_ids([[7]], max_tokens=9)                        # set_stops on a row with strings: ring and cut_bytes start afresh as well
    assert row.run([1, 0, 1]) == [(RUNNING, 1, 0), (RUNNING, 2, 0), (TEXT0, 3, 3)]
    row.set_ids([[7]], max_tokens=9)
    assert row.draw(1) == (RUNNING, 1, 0)                   # (cut_bytes is 0 again)


def test_stop_text_helper_builds_the_structure():
    st = g.stop_text([b"User:", "\n\n"])
    assert (st.n, list(st.len)[:3], bytes(st.bytes[0])[:5], bytes(st.bytes[1])[:2]) == (2, [5, 2, 0], b"User:", b"\n\n")
    assert C.sizeof(g.StopText) == 4 + 4 * 16 + 16 * 32 and g.STOP_TEXT0 == 16 == g.STOP_MAX_SEQS
    for bad in ([b"x"] * 17, [b"x" * 33], [b""]):
        with pytest.raises(ValueError):
            g.stop_text(bad)
    assert g.stop_text(["é" * 16]).len[0] == 32             # (bytes, not characters)


def test_every_case_again_under_the_sanitizers(H, tmp_path):
    """the harness as a program of its own with AddressSanitizer and UBSan replays every operation of the tests above (run once more
    here, to log them) and finds the same outcomes, every token's bytes in a heap buffer of exactly their length"""
    del H.cases[:]
    for case in (test_random_streams_match_the_restated_rule, test_match_spanning_three_tokens, test_match_wholly_inside_a_130_byte_token,
                 test_two_strings_completing_at_the_same_byte_lowest_k, test_a_higher_k_completing_earlier_in_the_token_wins,
                 test_a_string_longer_than_the_drawn_text_cannot_match, test_id_sequence_and_text_on_the_same_draw_id_wins,
                 test_text_and_budget_on_the_same_draw_text_wins, test_reset_by_either_setter):
        case(H)
    assert sum(1 for c in H.cases if c[0] == 4) >= 3000
    exe, cases = str(tmp_path / "stop_text_asan"), str(tmp_path / "cases.txt")
    subprocess.check_call(GXX + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DSTOP_TEXT_MAIN", "-o", exe, HARNESS])
    with open(cases, "w") as f:
        f.write("\n".join(" ".join(str(int(x)) for x in c) for c in H.cases) + "\n")
    r = subprocess.run([exe, cases], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 mismatches" in r.stdout
