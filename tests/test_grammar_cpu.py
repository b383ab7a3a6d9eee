"""CPU: constrained decoding's host side. The regular-expression compiler of the package (ggllm.cpp_amd/grammar.py) against Python's re on
every short byte string, and the rule the device compiles (ggllm.cpp_amd/csrc/fq_grammar.h), host-compiled with g++
(tests/host/grammar_harness.cpp), against its restatement in tests/grammar_ref.py. Every grammar any test builds is also written to a
file of cases, which the same harness -- built as a program of its own with -fsanitize=address,undefined -- replays."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import ggllm_cpp_amd as g
import grammar_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "host", "grammar_harness.cpp")
GXX = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "ggllm.cpp_amd", "csrc")]

# ---------------------------------------------------------------------------------------------- 1. the regex compiler
AB = b"ab1_\n"          # four letters (a digit and the underscore among them, for \d and \w) and one byte outside: the one . does not match
# (pattern, alphabet, the pattern re is given if it differs). From every live prefix of up to 3 bytes an accepted string lies within 3 more
# bytes of the alphabet, so "live" can be decided by brute force over strings of up to 6 bytes.
PATTERNS = [
    (b"a", AB), (b"ab|1", AB), (b"(ab|1_)+a", AB), (b"a*", AB), (b"a+b?", AB), (b"(a|b)*1", AB), (b"a{3}", AB), (b"a{2,4}", AB),
    (b"a{2,}b", AB), (b"[ab]{6}", AB), (b"a{0}b", AB), (b"(a|b){2}1{0,1}", AB), (b"[^a]b", AB), (b".a", AB), (b".*", AB), (b"\\d+", AB),
    (b"\\w\\s\\w", AB), (b"[a\\d]*_", AB), (b"[a-b1]+", AB), (b"[^ab\\n]{1,2}", AB), (b"a\\nb", AB), (b"\\x61\\x0a?", AB),
    (b"(a(b(1)?)?)?", AB), (b"a|", AB), (b"()a", AB), (b"(_|1)?(a|b)*_", AB), (b"[\\s\\w]?a", AB), (b"[ab]*a[ab]", AB), (b"[^\\d_]", AB),
    (b"\\.\\*\\\\?", b".*a\\b"), (b"[-a]b", b"-ab1\n"), (b"[a\\-b]+", b"-ab1\n"), (b"[a-]+", b"-ab1\n"), (b"a\\tb|\\t\\r?", b"ab\t\r\n"),
    (b"\\x00\\xff*", bytes([0, 255, 97, 98, 10])), (b"\\(a\\)\\|", b"()a|b"), (b"\\{a\\}\\[\\]", b"{}[]a"),
    ("é+a", b"\xc3\xa9ab\n", b"(\xc3\xa9)+a"),
]


def strings_upto(alphabet, n):
    for l in range(n + 1):
        for t in itertools.product(alphabet, repeat=l):
            yield bytes(t)


@pytest.mark.parametrize("case", PATTERNS, ids=[repr(p[0]) for p in PATTERNS])
def test_regex_dfa_equals_re_fullmatch_on_every_short_string(case):
    pattern, alphabet = case[0], case[1]
    rx = re.compile(case[2] if len(case) > 2 else pattern)
    d = g.regex_dfa(pattern)
    assert d.start == 1 and not d.trans[0].any() and not d.accept[0] and d.trans.max() < d.n_states
    accepted = set()
    state_of = {}
    for s in strings_upto(alphabet, 6):
        st = d.walk(state_of[s[:-1]], s[-1:]) if s else d.start      # (one step from the prefix's state)
        state_of[s] = st
        want = rx.fullmatch(s) is not None
        assert bool(d.accept[st]) == want, (pattern, s)
        if want:
            accepted.add(s)
    prefixes = {s[:k] for s in accepted for k in range(len(s) + 1)}
    for s in strings_upto(alphabet, 3):
        assert (state_of[s] != 0) == (s in prefixes), (pattern, s)
    assert d.accepts(b"") == (rx.fullmatch(b"") is not None) and d.live(b"") == bool(accepted)


def test_regex_dfa_is_minimal_and_trimmed():
    assert g.regex_dfa(b"(ab|cd)+x").n_states == 6          # dead, start, a, c, after a pair, accepted
    assert g.regex_dfa(b"[ab]{698}").n_states == 700        # dead, the start and 698 more
    assert g.regex_dfa(b"a|a|a").n_states == 3
    assert g.regex_dfa(b"(a|b)*").n_states == 2
    d = g.choice_dfa([b"yes", b"no", "yes"])
    assert d.n_states == 6 and d.accepts(b"yes") and d.accepts(b"no") and not d.accepts(b"ye") and d.live(b"ye") and not d.live(b"nos")
    assert g.choice_dfa([b"", b"a"]).accepts(b"")
    for d in (g.regex_dfa(b"(ab|cd)+x"), g.choice_dfa([b"abc", b"abd", b"x"])):
        # every state but 0 is reachable and reaches an accepting state
        for s in range(1, d.n_states):
            seen, todo = {s}, [s]
            while todo:
                for t in set(d.trans[todo.pop()].tolist()) - seen - {0}:
                    seen.add(t)
                    todo.append(t)
            assert any(d.accept[t] for t in seen)


@pytest.mark.parametrize("pattern", [b"a**", b"a*?", b"a++", b"a?+", b"a{2}{3}", b"(?:a)", b"(?P<n>a)", b"^a", b"a$", b"\\b", b"\\D", b"\\W", b"\\S", b"\\1", b"\\A",
                                     b"\\z", b"[a", b"(a", b"a)", b"a{2", b"a{,2}", b"a{3,2}", b"a{}", b"a{x}", b"[]a]", b"[b-a]", b"*a", b"|*", b"a]", b"a}",
                                     b"\\xg1", b"\\x1", b"[\\d-a]", b"[a-\\d]", b"[[a]", "[é]", "\\é", b"\\", b"[^\\x00-\\xff]", b"a[^\\x00-\\xff]"])
def test_regex_dfa_raises_on_what_it_does_not_know(pattern):
    with pytest.raises(ValueError):
        g.regex_dfa(pattern)


def test_dfa_constructor_checks_the_table():
    d = g.regex_dfa(b"ab")
    assert g.dfa(d.trans, d.accept, d.start).n_states == d.n_states
    bad = d.trans.copy()
    bad[1, 5] = d.n_states
    with pytest.raises(ValueError):
        g.dfa(bad, d.accept)
    bad = d.trans.copy()
    bad[0, 5] = 1
    with pytest.raises(ValueError):
        g.dfa(bad, d.accept)
    with pytest.raises(ValueError):
        g.dfa(d.trans, d.accept, start=d.n_states)
    with pytest.raises(ValueError):
        g.dfa(d.trans[:, :255], d.accept)
    with pytest.raises(ValueError):
        g.choice_dfa([])


# ---------------------------------------------------------------------------------------------- 2. fq_grammar.h
@pytest.fixture(scope="module")
def H(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("grammar") / "libgrammar_host.so")
    subprocess.check_call(GXX + ["-O2", "-fPIC", "-shared", "-o", out, HARNESS])
    L = C.CDLL(out)
    vp = C.c_void_p
    L.gr_walk.argtypes = [vp, C.c_int, vp, C.c_int]
    L.gr_allowed.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]
    L.gr_advance.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp]
    L.gr_build.argtypes = [C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    L.cases = []
    return L


def build(H, d, vocab, eos_id, n_states=None, start=None, steps=0, seed=0):
    """creation through the header next to the restatement: (code, bad state, index or None); every result asserted equal and logged"""
    n_states = d.n_states if n_states is None else n_states
    start = d.start if start is None else start
    trans, accept = np.ascontiguousarray(d.trans), np.ascontiguousarray(d.accept)
    pool, offs = ref.pool_of(vocab)
    V, W = len(vocab), (len(vocab) + 63) // 64
    assert H.gr_words(V) == W
    index, counts, bad = np.zeros((max(n_states, 1), W), np.uint64), np.zeros(max(n_states, 1), np.int32), C.c_int(-9)
    code = H.gr_build(n_states, start, trans.ctypes.data, accept.ctypes.data, V, eos_id, pool.ctypes.data, offs.ctypes.data, index.ctypes.data, counts.ctypes.data, C.byref(bad))
    want = ref.check(n_states, start, trans, accept, eos_id, vocab)
    assert (code, bad.value) == want
    have_index = code in (ref.OK, ref.DEAD_END)
    log = [n_states, start, V, eos_id, int(offs[-1])] + trans[:max(n_states, 0)].ravel().tolist() + accept[:max(n_states, 0)].tolist() + offs.tolist() + pool[:int(offs[-1])].tolist()
    log += [code, bad.value, 1 if have_index else 0]
    if have_index:
        want_index = ref.index(trans, accept, eos_id, vocab)
        assert np.array_equal(index, want_index)
        assert not index[0].any()
        if V % 64:
            assert not (index[:, -1] >> np.uint64(V % 64)).any()        # bits at and beyond n_vocab
        assert counts.tolist() == [sum(bin(int(x)).count("1") for x in row) for row in index]
        log += index.ravel().view(np.int64).tolist()
    rng = np.random.default_rng(seed)
    log.append(steps if code == ref.OK else 0)
    if code == ref.OK:
        state = start
        for _ in range(steps):
            t = int(rng.integers(0, V))
            a = H.gr_allowed(trans.ctypes.data, accept.ctypes.data, state, t, eos_id, pool.ctypes.data, offs.ctypes.data)
            nx = H.gr_advance(trans.ctypes.data, state, t, eos_id, pool.ctypes.data, offs.ctypes.data)
            assert a == int(ref.allowed(trans, accept, state, t, eos_id, vocab)) and nx == ref.advance(trans, state, t, eos_id, vocab)
            assert a == int((int(index[state, t // 64]) >> (t % 64)) & 1)
            assert H.gr_walk(trans.ctypes.data, state, pool[offs[t]:].ctypes.data if offs[t] < len(pool) else pool.ctypes.data, len(vocab[t])) == ref.walk(trans, state, vocab[t])
            log += [state, t, a, nx]
            state = nx if a else (start if rng.integers(0, 4) == 0 else state)         # follow allowed tokens, sometimes start over
    H.cases.append(log)
    return code, bad.value, index if have_index else None


@pytest.fixture(scope="module")
def vocabs():
    rng = np.random.default_rng(11)
    v300 = ref.vocab300(rng)
    return v300, v300[:65]


@pytest.mark.parametrize("n_vocab", [300, 65])
def test_header_equals_restatement(H, vocabs, n_vocab):
    vocab = vocabs[0] if n_vocab == 300 else vocabs[1]
    assert sorted({len(b) for b in vocab} & {0, 1, 63, 64, 65, 130}) == [0, 1, 63, 64, 65, 130] and vocab[1] == b"\0" and vocab[2] == b"\xff"
    eos = 0                                                  # the token without bytes plays EOS: allowed by accept alone
    for k, pattern in enumerate([b"[abcd]*", b"(ab|cd)+", b"[abcd]{0,70}", b"\\x00\\xff*[ab]?", b"a(b|c)d*", b"ab"]):
        d = g.regex_dfa(pattern)
        code, bad, index = build(H, d, vocab, eos, steps=200, seed=k)
        assert code == ref.OK
        for s in range(1, d.n_states):                       # EOS in accepting and non-accepting states
            assert bool(index[s, 0] & np.uint64(1)) == bool(d.accept[s])
    # an accepting state without outgoing transitions: only EOS is allowed there
    d = g.regex_dfa(b"ab")
    code, bad, index = build(H, d, vocab, eos, steps=50)
    last = d.walk(d.start, b"ab")
    assert code == ref.OK and d.accept[last] and not d.trans[last].any() and index[last].tolist() == [1] + [0] * (len(index[last]) - 1)
    # ... and without an EOS token that state allows nothing: refused with its number
    assert build(H, d, vocab, -1)[:2] == (ref.DEAD_END, last)
    # a token without bytes that is not EOS is never allowed, a long token inside a short automaton is not either
    d = g.regex_dfa(b"[abcd]{0,70}")
    index = build(H, d, vocab, -1)[2]
    assert not (index[:, 0] & np.uint64(1)).any()
    t130 = [t for t, b in enumerate(vocab) if len(b) == 130][0]
    assert not (index[:, t130 // 64] >> np.uint64(t130 % 64) & np.uint64(1)).any()
    t65 = [t for t, b in enumerate(vocab) if len(b) == 65][0]
    assert int(index[d.start, t65 // 64] >> np.uint64(t65 % 64) & np.uint64(1)) == 1 and d.walk(d.start, vocab[t65]) != 0


def test_header_refusals(H, vocabs):
    vocab = vocabs[0]
    d = g.regex_dfa(b"az")                                   # no token holds a z: the state after a allows nothing
    assert build(H, d, vocab, 0)[:2] == (ref.DEAD_END, d.walk(d.start, b"a"))
    d = g.regex_dfa(b"(ab|cd)+")
    bad = g.Dfa(d.trans.copy(), d.accept, d.start)
    bad.trans[3, 200] = d.n_states                           # a transition out of range, the state whose row holds it
    assert build(H, bad, vocab, 0)[:2] == (ref.BAD_TRANS, 3)
    bad = g.Dfa(d.trans.copy(), d.accept, d.start)
    bad.trans[0, 97] = 1                                     # out of the dead state
    assert build(H, bad, vocab, 0)[:2] == (ref.BAD_TRANS, 0)
    assert build(H, d, vocab, 0, start=d.n_states)[:2] == (ref.BAD_ARGS, -1)
    assert build(H, d, vocab, len(vocab))[:2] == (ref.BAD_ARGS, -1)
    assert build(H, d, vocab, 0, n_states=0)[:2] == (ref.BAD_ARGS, -1)


def test_zz_sanitized_replay_of_every_case(H, tmp_path):
    """the harness as a program of its own under AddressSanitizer and UBSan, over every grammar the tests above built"""
    assert len(H.cases) >= 20
    exe, cases = str(tmp_path / "grammar_harness"), str(tmp_path / "cases.bin")
    subprocess.check_call(GXX + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DGRAMMAR_HARNESS_MAIN", "-o", exe, HARNESS])
    np.array([x for c in H.cases for x in c], np.int64).tofile(cases)
    r = subprocess.run([exe, cases], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d cases" % len(H.cases) in r.stdout
