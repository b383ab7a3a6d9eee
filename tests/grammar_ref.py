"""The constraint rule of ggllm.cpp_amd/csrc/fq_grammar.h restated in Python, for tests/test_grammar_cpu.py (against the header compiled
with g++) and tests/test_gpu_grammar.py (against the device): walk, allowed, the index, the creation check, and the logits row a
constrained draw is equivalent to (a -inf on every forbidden token)."""
import numpy as np

OK, BAD_ARGS, BAD_TRANS, DEAD_END = 0, 1, 2, 3
MAX_STATES = 16384


def walk(trans, state, data):
    for b in bytes(data):
        if state == 0:
            return 0
        state = int(trans[state][b])
    return state


def allowed(trans, accept, state, token, eos_id, vocab):
    if state == 0:
        return False
    if token == eos_id:
        return bool(accept[state])
    return len(vocab[token]) > 0 and walk(trans, state, vocab[token]) != 0


def advance(trans, state, token, eos_id, vocab):
    return state if token == eos_id else walk(trans, state, vocab[token])


def allowed_row(trans, accept, state, eos_id, vocab):
    """bool [n_vocab]: which tokens the state allows"""
    return np.array([allowed(trans, accept, state, t, eos_id, vocab) for t in range(len(vocab))], bool)


def index(trans, accept, eos_id, vocab):
    """uint64 [n_states][ceil(n_vocab / 64)]: bit t % 64 of word t / 64 set exactly when t is allowed; bits at and beyond n_vocab 0.
    One walk per (first byte's target, token) would be faster; this is the definition, computed by distinct token bytes"""
    trans = np.asarray(trans).tolist()                      # (plain lists: the walks below are the test's whole cost)
    n, V = len(trans), len(vocab)
    W = (V + 63) // 64
    out = np.zeros((n, W), np.uint64)
    distinct = {}
    for t, b in enumerate(vocab):
        distinct.setdefault(bytes(b), []).append(t)
    for s in range(1, n):
        for b, toks in distinct.items():
            ok = len(b) > 0 and walk(trans, s, b) != 0
            for t in toks:
                if (bool(accept[s]) if t == eos_id else ok):
                    out[s, t // 64] |= np.uint64(1) << np.uint64(t % 64)
    return out


def check(n_states, start, trans, accept, eos_id, vocab):
    """(code, state to blame or -1) of creating this grammar"""
    V = len(vocab)
    if not 1 <= n_states <= MAX_STATES or not 0 <= start < n_states or V < 1 or not -1 <= eos_id < V:
        return BAD_ARGS, -1
    for s in range(n_states):
        for b in range(256):
            to = int(trans[s][b])
            if to >= n_states or (s == 0 and to != 0):
                return BAD_TRANS, s
    for s in range(1, n_states):
        if not any(allowed(trans, accept, s, t, eos_id, vocab) for t in range(V)):
            return DEAD_END, s
    return OK, -1


def masked(logits, allow):
    """the row an unconstrained sampler must be given to draw what the constrained one draws: -inf where the token is forbidden"""
    x = np.array(logits, np.float32, copy=True)
    x[~allow] = -np.inf
    return x


def pool_of(vocab):
    offs = np.zeros(len(vocab) + 1, np.int32)
    offs[1:] = np.cumsum([len(b) for b in vocab])
    pool = np.frombuffer(b"".join(vocab) or b"\0", np.uint8).copy()
    return pool, offs


def vocab300(rng):
    """300 tokens over a, b, c, d and the bytes 0 and 255: lengths 0, 1, 63, 64, 65 and 130 among them, the rest short; ids 1 and 2 are the
    single bytes 0 and 255"""
    lens = [0, 1, 1, 63, 64, 65, 130] + [int(x) for x in rng.integers(1, 5, 293)]
    v = [bytes(rng.integers(97, 101, l, dtype=np.uint8)) for l in lens]
    v[1], v[2] = b"\x00", b"\xff"
    v[7], v[8], v[9], v[10] = b"a", b"b", b"c", b"d"
    return v
