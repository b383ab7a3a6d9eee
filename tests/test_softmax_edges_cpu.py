"""CPU: the soft-max edge cases of tests/softmax_edges.py -- what test_gpu_softmax_edges.py holds the attention kernels to -- are what they claim to be:
their numpy expectation is the oracle's soft_max bit for bit, the sweep really produces every table index 0x8000 .. 0xFC00 in both constructions, every
compared output element has exactly one non-zero V term, and a soft-max with one of the faults the families aim at changes an observed element."""
import numpy as np
import pytest

import softmax_edges as se

FIX = se.fix_list_from_header()
FIX_BITS = se.reachable(FIX)
N_IDX = se.IDX_LAST - se.IDX_FIRST + 1
PREFILL = ([("S", (n_past, 64)) for n_past in se.S_N_PAST] + [("T", (65, 64)), ("R", (65, 64)), ("W", (se.W_N16 + 1, 64)), ("W", (3500, 64)), ("M", (65, 64)),
           ("M", (0, 64)), ("M", (3500, 64))] + [("U", (n_kv, 33)) for n_kv in se.U_SIZES] + [("U", (n_kv, 1)) for n_kv in se.U_SIZES])
SEQS = {route: len(r[1]) for route, r in se.DECODE_ROUTES.items()}
SWEEP_ROUTES = [route for route in se.DECODE_ROUTES if SEQS[route] == se.N_SEQ]
DECODE = ([("S", route, launch) for route in SWEEP_ROUTES for launch in range(se.DEC_SWEEP_LAUNCHES)] +
          [(name, route, launch) for route in se.DECODE_ROUTES for name in "TW" for launch in range(se.t_launches(FIX, SEQS[route]))])


@pytest.fixture(scope="module")
def tab(oracle):
    return se.table_f32(oracle)


@pytest.fixture(scope="module")
def cases():
    memo = {}

    def get(family, args):
        if (family, args) not in memo:
            memo[family, args] = (se.family_S(FIX, *args) if family == "S" else se.family_T(FIX, *args) if family == "T" else
                                  {"R": se.family_R, "W": se.family_W, "M": se.family_M, "U": se.family_U}[family](*args))
        return memo[family, args]
    return get


@pytest.fixture(scope="module")
def decodes(oracle):
    memo = {}

    def get(name, route, launch=0):
        if (name, route, launch) not in memo:
            _, positions, obs0, _ = se.DECODE_ROUTES[route]
            memo[name, route, launch] = (se.decode_family(oracle, name, FIX, positions, obs0, launch), obs0)
        return memo[name, route, launch]
    return get


def test_the_measured_table_entries(oracle):
    """the facts the families are built on: the first subnormal and the first zero result, the entries at the formula's thresholds"""
    t = oracle.exp_table()
    assert t[se.SUBNORMAL_FIRST - 1] >= 0x0400 and 0 < t[se.SUBNORMAL_FIRST] < 0x0400 and t[se.ZERO_FIRST - 1] == 1 and t[se.ZERO_FIRST] == 0
    assert (t[se.SUBNORMAL_FIRST:se.ZERO_FIRST] > 0).all() and (t[se.SUBNORMAL_FIRST:se.ZERO_FIRST] < 0x0400).all() and se.ZERO_FIRST - se.SUBNORMAL_FIRST == 891
    assert [int(t[b]) for b in (0xCC00, 0xCC0E, 0xCC0F, 0xCC55, 0xFBFF, 0xFC00)] == [2, 2, 1, 1, 0, 0]
    assert t[0x8000] == 0x3C00 and t[0xCC40] == 1          # -0 -> 1.0; -17.0 -> 2^-24 (family W's type 13)
    assert len(FIX) == 48 and all(int(t[b]) == e for b, e in FIX) and len(FIX_BITS) == 21


@pytest.mark.parametrize("family,args", PREFILL, ids=[f"{f}@{a[0]}x{a[1]}" for f, a in PREFILL])
def test_prefill_expectation_is_the_oracles_soft_max(oracle, tab, cases, family, args):
    """every row of every family, masked keys at -inf: equal bit for bit; and every compared output element has exactly one non-zero V term, every other
    element none"""
    c = cases(family, args)
    N = c.n_max
    s, vis = c.scores(N)
    vis = np.broadcast_to(vis, s.shape)
    p, _ = se.soft_max(tab, s, vis)
    ref = oracle.softmax_rows(np.where(vis, s, -np.inf).astype(np.float32))
    assert np.array_equal(p * vis, ref)
    terms = np.cumsum(c.vc != 0, axis=0)[c.n_past + np.arange(N)]                 # [N, H, D]: non-zero V[j][h][d] over the keys row t sees
    obs = c.observed(N)
    assert np.array_equal(terms, np.broadcast_to(obs[:, None, :], terms.shape).astype(terms.dtype))
    assert (obs.sum(axis=1) == np.minimum(se.D, c.n_past + 1 + np.arange(N) - c.obs0)).all()      # no visible key among obs0 .. obs0 + 63 is left out
    out, _ = c.expected(tab, N)
    n_obs = min(se.D, s.shape[-1] - c.obs0)
    assert np.array_equal(out.reshape(N, se.H, se.D)[:, :, :n_obs], ref[:, :, c.obs0:c.obs0 + n_obs] * obs[:, None, :n_obs]) and np.isfinite(out).all()


@pytest.mark.parametrize("name,route,launch", DECODE, ids=[f"{n}-{r}-{l}" for n, r, l in DECODE])
def test_decode_expectation_is_the_oracles_soft_max(oracle, tab, decodes, name, route, launch):
    cs, obs0 = decodes(name, route, launch)
    for c, s in cs:
        p, _ = se.soft_max(tab, s, np.ones(s.shape, bool))
        assert np.array_equal(p, oracle.softmax_rows(s))
        assert np.array_equal((c.values() != 0).sum(axis=0), np.ones((se.H, se.D), np.int64))      # one non-zero V term per output element
        # the construction's premises: one non-zero product per K.Q, the new key scores 0
        assert ((c.keys() != 0).sum(axis=2) <= 1).all() and not c.k_new.any() and (s[:, -1] == 0).all()
        prod = (c.q_rot[None] * c.keys()).astype(np.float32).astype(np.float64).sum(axis=2).astype(np.float32) * np.float32(0.125)
        assert np.array_equal(prod.T, s)


def _prefill_indices(c, tab, N, c0=0):
    _, idx = c.expected(tab, N, c0)
    return idx[:, :, c.obs0:c.obs0 + se.D]


def test_sweep_coverage_prefill(tab, cases):
    """S: 31745 of 31745 indices among the OBSERVED slots of one launch, counted from the scores the builder emits -- at every n_past the GPU test uses"""
    for n_past in se.S_N_PAST:
        idx = _prefill_indices(cases("S", (n_past, 64)), tab, 64)
        seen = np.unique(idx)
        assert seen.size == N_IDX and seen[0] == se.IDX_FIRST and seen[-1] == se.IDX_LAST, (n_past, seen.size)
    # N = 31 in three launches rotating the components
    c = cases("S", (65, 64))
    seen = np.unique(np.concatenate([_prefill_indices(c, tab, 31, c0).ravel() for c0 in range(0, se.D, 31)]))
    assert seen.size == N_IDX


@pytest.mark.parametrize("route", SWEEP_ROUTES)
def test_sweep_coverage_decode(tab, decodes, route):
    seen = set()
    for launch in range(se.DEC_SWEEP_LAUNCHES):
        cs, obs0 = decodes("S", route, launch)
        for _, s in cs:
            seen.update(se.decode_expected(tab, s, obs0)[1][:, obs0:obs0 + se.DEC_OBS].ravel().tolist())
    assert len(seen) == N_IDX and min(seen) == se.IDX_FIRST and max(seen) == se.IDX_LAST, len(seen)


def test_targeted_coverage(tab, cases, decodes):
    """T: every reachable fix-list input, the 891 subnormal results and the thresholds, in the two components a short launch reads and in one decode launch"""
    want = set(FIX_BITS) | set(range(se.SUBNORMAL_FIRST, se.ZERO_FIRST)) | set(se.THRESHOLDS)
    assert len(want) == 21 + 891 + 5                       # (0xCC00, 0xCC0E, 0xCC0F and 0xCC55 lie in the band)
    c = cases("T", (65, 64))
    assert want <= set(_prefill_indices(c, tab, se.T_COMPONENTS).ravel().tolist())
    assert want <= set(np.concatenate([_prefill_indices(c, tab, 1, c0).ravel() for c0 in range(se.T_COMPONENTS)]).tolist())
    for route in se.DECODE_ROUTES:
        seen = set()
        for launch in range(se.t_launches(FIX, SEQS[route])):
            cs, obs0 = decodes("T", route, launch)
            for _, s in cs:
                seen.update(se.decode_expected(tab, s, obs0)[1][:, obs0:obs0 + se.DEC_OBS].ravel().tolist())
            cs, obs0 = decodes("W", route, launch)         # the cached maximum of +16.25: the new key's result is the subnormal 1, observed in element 63
            for _, s in cs:
                out, idx = se.decode_expected(tab, s, obs0)
                assert (idx[:, -1] == 0xCC10).all() and (out.reshape(se.H, se.D)[:, -1] > 0).all() and (s.max(axis=1) == s[:, 0]).all()
        assert want <= seen, route


def test_r_pairs_part_the_two_roundings(tab, cases):
    """every R pair: f32(s - m) is the fp16 tie, one rounding of the exact difference gives the other neighbour; wherever the two neighbours' table entries
    differ (at least 64 pairs: below 2.4e-4 every entry is 1.0, beyond 17.33 every entry is 0) the probability differs too. Subnormal inputs included."""
    c = cases("R", (65, 64))
    m, s = c.pairs
    two = (s - m).astype(np.float16).view(np.uint16)
    one = (s.astype(np.float64) - m.astype(np.float64)).astype(np.float16).view(np.uint16)
    assert (s.astype(np.float64) - m.astype(np.float64) != (s - m).astype(np.float64)).all()          # s - m is not an f32
    assert ((s - m) == -m).all() and (np.abs(one.astype(int) - two.astype(int)) == 1).all() and (two & 1 == 0).all()
    assert ((two & 0x7C00) == 0).sum() >= 8                # fp16-subnormal differences
    assert np.unique(two >> 10).size == 31                 # every binade
    good, _ = c.expected(tab, 64)
    bad, _ = c.expected(tab, 64, fault="single")
    g0, b0 = good.reshape(64, se.H, se.D)[:, :, 0].T.ravel(), bad.reshape(64, se.H, se.D)[:, :, 0].T.ravel()          # observed key 1 holds the pair's s; [h * 64 + c]
    entries_differ = tab[one] != tab[two]
    assert entries_differ.sum() >= 64 and (g0 != b0)[entries_differ].all()


def _changed(c, tab, fault, N=64, c0=0):
    good, _ = c.expected(tab, N, c0)
    bad, _ = c.expected(tab, N, c0, fault, FIX_BITS)
    return int((good != bad).sum())


def test_the_expectations_bite(tab, cases, decodes):
    """a soft-max with the named fault changes at least one observed element of the family aimed at it"""
    assert _changed(cases("R", (65, 64)), tab, "single") > 0
    assert _changed(cases("R", (65, 64)), tab, "single", 1, 1) > 0 and _changed(cases("R", (65, 64)), tab, "single", 3, 0) > 0      # (the short routes' launches)
    assert _changed(cases("R", (3500, 64)), tab, "single", 16, 0) > 0
    assert _changed(cases("T", (65, 64)), tab, "ftz", se.T_COMPONENTS) > 0 and _changed(cases("W", (se.W_N16 + 1, 64)), tab, "ftz") > 0
    assert _changed(cases("W", (se.W_N16 + 1, 64)), tab, "f32sum") > 0
    assert _changed(cases("M", (65, 64)), tab, "leak") > 0 and _changed(cases("M", (0, 64)), tab, "leak") > 0
    assert _changed(cases("T", (65, 64)), tab, "offby1", se.T_COMPONENTS) > 0
    assert _changed(cases("S", (65, 64)), tab, "ftz") > 0 and _changed(cases("S", (65, 64)), tab, "offby1") > 0
    # row 0 of M at n_past 0 sees one key: p = 1; with the leak the +30000 key takes everything
    c = cases("M", (0, 64))
    assert (c.expected(tab, 64)[0][0].reshape(se.H, se.D)[:, 0] == 1.0).all() and (c.expected(tab, 64, fault="leak")[0][0].reshape(se.H, se.D)[:, 0] == 0.0).all()
    cs, obs0 = decodes("T", "same_65")
    for fault in ("ftz", "offby1"):
        assert any((se.decode_expected(tab, s, obs0)[0] != se.decode_expected(tab, s, obs0, fault, FIX_BITS)[0]).any() for _, s in cs)
    cs, obs0 = decodes("W", "same_65")
    assert all(se.decode_expected(tab, s, obs0)[0][se.D - 1] != se.decode_expected(tab, s, obs0, "ftz")[0][se.D - 1] for _, s in cs)


def test_uniform_and_wide_rows(tab, cases):
    """U: p = f32(1 / visible keys) in every observed element; W's -16.0 row sums to 1 + 4600 x 2^-24 and its probabilities are 2 x 2^-24 x inv"""
    for n_kv in se.U_SIZES:
        c = cases("U", (n_kv, 33))
        out, _ = c.expected(tab, 33)
        want = np.float32(1.0) * (1.0 / (c.n_past + 1 + np.arange(33))).astype(np.float32)
        assert (out.reshape(33, se.H, se.D) == want[:, None, None] * c.observed(33)[:, None, :]).all()
        assert c.n_past + 33 == max(n_kv, 33)
    c = cases("W", (se.W_N16 + 1, 64))
    out, _ = c.expected(tab, 64)
    inv = np.float32(1.0 / (1.0 + 2 * se.W_N16 * 2.0 ** -24))
    assert (out.reshape(64, se.H, se.D)[12] == np.float32(2.0 ** -23) * inv).all()
    assert (out.reshape(64, se.H, se.D)[13] == np.float32(2.0 ** -24) * np.float32(1.0 / (1.0 + se.W_N16 * 2.0 ** -24))).all()
