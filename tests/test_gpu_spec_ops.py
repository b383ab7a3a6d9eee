"""GPU: the two operators of draft-and-verify decode on caller-made data (include/ggml-hip-ops.h, csrc/kernels_sample.hip).
ggml_hip_draft_lookup against tests/spec_ref.py; ggml_hip_sampler_verify_rows against ggml_hip_sampler_sample run row by row on
a second sampler for the same number of draws: the same draws, generator, mu and stop state, and -- since the ABI has no window
getter -- the same three further draws with penalties that depend on the window."""
import ctypes as C

import numpy as np
import pytest

import ggllm_cpp_amd as g
import sample_ref
import spec_ref as sr

pytestmark = pytest.mark.gpu

V, ROWS = 300, 5


@pytest.fixture(scope="module")
def L():
    L = g.load()
    L.ggml_hip_init(0)
    return L


# ---------------------------------------------------------------------------------------------- ggml_hip_draft_lookup
def device_lookup(L, bufs, h, gmin, gmax, K):
    hd, dd = bufs
    a = np.ascontiguousarray(h, np.int32)
    out = np.full(15, -7, np.int32)
    if a.size:
        L.ggml_hip_memcpy_h2d(hd, a.ctypes.data, a.nbytes)
    L.ggml_hip_memcpy_h2d(dd, out.ctypes.data, out.nbytes)
    assert L.ggml_hip_draft_lookup(hd, a.size, gmin, gmax, K, dd) == 0
    L.ggml_hip_memcpy_d2h(out.ctypes.data, dd, out.nbytes)
    L.ggml_hip_synchronize()
    assert (out[K:] == -7).all()                                # nothing written behind the K drafts
    return out[:K].tolist()


@pytest.fixture(scope="module")
def bufs(L):
    hd, dd = L.ggml_hip_malloc(4096 * 4), L.ggml_hip_malloc(64)
    yield hd, dd
    L.ggml_hip_free(hd)
    L.ggml_hip_free(dd)


def test_lookup_by_hand(L, bufs):
    for name, h, gmin, gmax, K, want in sr.LOOKUP_CASES:
        assert device_lookup(L, bufs, h, gmin, gmax, K) == want, name


def test_lookup_random_histories(L, bufs):
    """200 histories over an alphabet of 4 (matches of every length abound), n from 1 to 64; and one longer than the workgroup"""
    rng = np.random.default_rng(17)
    for i in range(200):
        n = 1 + i % 64
        h = rng.integers(0, 4, n).tolist()
        gmin = int(rng.integers(1, 4))
        gmax = gmin + int(rng.integers(0, 4))
        K = int(rng.integers(1, 16))
        assert device_lookup(L, bufs, h, gmin, gmax, K) == sr.lookup(h, gmin, gmax, K), (h, gmin, gmax, K)
    h = rng.integers(0, 7, 3000).tolist()                       # 3 ends per thread: the strided scan and the reduction across all 16 waves
    for gmin, gmax in ((1, 3), (4, 8), (6, 32)):
        assert device_lookup(L, bufs, h, gmin, gmax, 15) == sr.lookup(h, gmin, gmax, 15)


def test_lookup_refusals(L, bufs):
    hd, dd = bufs
    for n, gmin, gmax, K in ((-1, 1, 3, 3), (8, 0, 3, 3), (8, 3, 2, 3), (8, 1, 33, 3), (8, 1, 3, 0), (8, 1, 3, 16)):
        assert L.ggml_hip_draft_lookup(hd, n, gmin, gmax, K, dd) == 1
    assert L.ggml_hip_draft_lookup(hd, 8, 1, 3, 3, None) == 1


# ---------------------------------------------------------------------------------------------- ggml_hip_sampler_verify_rows
def _window(rng):
    return [int(t) for t in rng.integers(0, V, 64)]


CHAINS = {
    "greedy": lambda: g.sampling_ext(temp=0.0, repeat_penalty=1.3, repeat_last_n=64, frequency_penalty=0.3, seed=3),
    "default": lambda: g.sampling_ext(temp=0.8, top_k=40, top_p=0.95, repeat_penalty=1.1, repeat_last_n=64, seed=21, logit_bias={5: 2.5}),
    "tail-free + typical": lambda: g.sampling_ext(tfs_z=0.95, typical_p=0.9, temp=0.9, top_k=200, top_p=0.95, repeat_penalty=1.1, repeat_last_n=64,
                                                  frequency_penalty=0.2, seed=22),
    "mirostat 2": lambda: g.sampling_ext(mirostat=2, mirostat_tau=3.0, mirostat_eta=0.5, temp=1.5, repeat_penalty=1.1, repeat_last_n=64, presence_penalty=0.5, seed=24),
}


class Row:
    """one sampler of one row, with ROWS logits rows on the device"""

    def __init__(self, L, p, window, rows, stops=None):
        self.L = L
        self.s = L.ggml_hip_sampler_create(1, V, 64)
        assert self.s
        h = np.ascontiguousarray(window, np.int32)
        assert L.ggml_hip_sampler_set_row_ext(self.s, 0, C.byref(p), h.ctypes.data, h.size) == 0
        if stops is not None:
            assert L.ggml_hip_sampler_set_stops(self.s, 0, C.byref(stops)) == 0
        x = np.ascontiguousarray(np.stack(rows), np.float32)
        self.lg = L.ggml_hip_malloc(x.nbytes)
        self.tk = L.ggml_hip_malloc(256)
        L.ggml_hip_memcpy_h2d(self.lg, x.ctypes.data, x.nbytes)

    def plain(self, row):
        """ggml_hip_sampler_sample on logits row `row`; -1 if the row's stops had ended it"""
        out = np.full(1, -1, np.int32)
        self.L.ggml_hip_memcpy_h2d(self.tk, out.ctypes.data, 4)
        self.L.ggml_hip_sampler_sample(self.s, self.lg + row * V * 4, V, self.tk)
        self.L.ggml_hip_memcpy_d2h(out.ctypes.data, self.tk, 4)
        self.L.ggml_hip_synchronize()
        return int(out[0])

    def verify(self, drafts, n_rows=ROWS):
        d = np.ascontiguousarray(drafts, np.int32)
        out = np.full(n_rows + 2, -9, np.int32)
        L = self.L
        L.ggml_hip_memcpy_h2d(self.tk, out.ctypes.data, out.nbytes)
        if d.size:
            L.ggml_hip_memcpy_h2d(self.tk + 128, d.ctypes.data, d.nbytes)
        assert L.ggml_hip_sampler_verify_rows(self.s, self.lg, V, n_rows, self.tk + 128, self.tk, self.tk + 64) == 0
        n = np.zeros(1, np.int32)
        L.ggml_hip_memcpy_d2h(out.ctypes.data, self.tk, out.nbytes)
        L.ggml_hip_memcpy_d2h(n.ctypes.data, self.tk + 64, 4)
        L.ggml_hip_synchronize()
        assert (out[n_rows:] == -9).all()                       # n_rows slots are written, no more
        assert (out[int(n[0]):n_rows] == -1).all()
        return out[:int(n[0])].tolist()

    def state(self):
        L = self.L
        words, pos = np.zeros(624, np.uint32), C.c_int32(0)
        assert L.ggml_hip_sampler_get_rng(self.s, 0, words.ctypes.data, C.addressof(pos)) == 0
        mu = np.zeros(1, np.float32)
        assert L.ggml_hip_sampler_get_mu(self.s, mu.ctypes.data) == 0
        nd, rs = np.zeros(1, np.int32), np.zeros(1, np.int32)
        assert L.ggml_hip_sampler_get_stops(self.s, nd.ctypes.data, rs.ctypes.data) == 0
        return words.tobytes(), pos.value, mu.view(np.uint32).item(), int(nd[0]), int(rs[0])

    def free(self):
        self.L.ggml_hip_free(self.lg)
        self.L.ggml_hip_free(self.tk)
        self.L.ggml_hip_sampler_free(self.s)


def _rows(seed):
    rng = np.random.default_rng(seed)
    return [sample_ref.tie_free_row(rng, V, 3.0) for _ in range(ROWS)], _window(rng)


def _other(t):
    return (t + 1) % V


@pytest.mark.parametrize("chain", list(CHAINS))
@pytest.mark.parametrize("n_match", [0, 2, 4])
def test_verify_equals_plain_sampling_row_by_row(L, chain, n_match):
    """drafts that are right for n_match rows: n_match + 1 draws, and everything the sampler holds is what n_match + 1 plain
    launches leave"""
    rows, window = _rows(100 + len(chain))
    truth_row = Row(L, CHAINS[chain](), window, rows)
    try:
        truth = [truth_row.plain(j) for j in range(ROWS)]
    finally:
        truth_row.free()
    drafts = list(truth[:ROWS - 1])
    if n_match < ROWS - 1:
        drafts[n_match] = _other(truth[n_match])
    a, b = Row(L, CHAINS[chain](), window, rows), Row(L, CHAINS[chain](), window, rows)
    try:
        got = a.verify(drafts)
        want = [b.plain(j) for j in range(n_match + 1)]
        assert got == want == truth[:n_match + 1]
        assert a.state() == b.state()
        # the window: three more draws, whose penalties read it
        assert [a.plain(j) for j in (4, 2, 0)] == [b.plain(j) for j in (4, 2, 0)]
        assert a.state() == b.state()
    finally:
        a.free()
        b.free()


def test_verify_missing_drafts_and_single_row(L):
    """a row without a draft (-1) is never accepted; a pass of one row is one plain draw"""
    rows, window = _rows(7)
    a, b = Row(L, CHAINS["default"](), window, rows), Row(L, CHAINS["default"](), window, rows)
    try:
        truth = [b.plain(0), b.plain(1)]
        assert a.verify([truth[0], -1, 1, 2]) == truth
        assert a.verify([], n_rows=1) == [b.plain(0)]
        assert a.state() == b.state()
    finally:
        a.free()
        b.free()


@pytest.mark.parametrize("chain", ["default", "mirostat 2"])
def test_verify_stops_at_the_draw_that_completes_a_stop_sequence(L, chain):
    """a stop sequence that the second draw completes: two draws although every draft is right, reason 0, and a further pass draws
    nothing and moves nothing"""
    rows, window = _rows(55)
    t = Row(L, CHAINS[chain](), window, rows)
    try:
        truth = [t.plain(j) for j in range(ROWS)]
    finally:
        t.free()
    st = g.stops([[truth[0], truth[1]]])
    a, b = Row(L, CHAINS[chain](), window, rows, st), Row(L, CHAINS[chain](), window, rows, st)
    try:
        assert a.verify(truth[:ROWS - 1]) == truth[:2]
        assert [b.plain(0), b.plain(1), b.plain(2)] == truth[:2] + [-1]
        assert a.state() == b.state() and a.state()[3:] == (2, 0)
        before = a.state()
        assert a.verify(truth[:ROWS - 1]) == []
        assert a.state() == before
    finally:
        a.free()
        b.free()


def test_verify_budget_of_the_stops(L):
    """max_tokens 3: the third draw ends the row with STOP_BUDGET, inside a pass whose drafts are all right"""
    rows, window = _rows(56)
    t = Row(L, CHAINS["default"](), window, rows)
    try:
        truth = [t.plain(j) for j in range(ROWS)]
    finally:
        t.free()
    a = Row(L, CHAINS["default"](), window, rows, g.stops(max_tokens=3))
    try:
        assert a.verify(truth[:ROWS - 1]) == truth[:3]
        assert a.state()[3:] == (3, g.STOP_BUDGET)
    finally:
        a.free()


def test_verify_refusals(L):
    rows, window = _rows(1)
    a = Row(L, CHAINS["default"](), window, rows)
    try:
        before = a.state()
        assert L.ggml_hip_sampler_verify_rows(a.s, a.lg, V, 0, a.tk + 128, a.tk, a.tk + 64) == 1
        assert L.ggml_hip_sampler_verify_rows(a.s, a.lg, V, 17, a.tk + 128, a.tk, a.tk + 64) == 1
        assert L.ggml_hip_sampler_verify_rows(a.s, a.lg, V, 3, None, a.tk, a.tk + 64) == 1
        assert L.ggml_hip_sampler_verify_rows(a.s, None, V, 3, a.tk + 128, a.tk, a.tk + 64) == 1
        assert a.state() == before
    finally:
        a.free()
