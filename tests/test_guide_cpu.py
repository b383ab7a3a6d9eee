"""CPU: the guidance arithmetic (csrc/fq_guide.h, through tests/host/guide_harness.cpp) against an independent numpy restatement
of the pinned summation order and the mix (tests/guide_ref.py) -- the double sums on 64 bits, every mixed value on 32 -- and
the pinned order told apart from the in-order chain of fq_score.h."""
import numpy as np
import pytest

import guide_ref as gr
import score_ref as sr

SCALES = [1.5, 1.0, 0.0, -0.5, 7.5]


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return gr.build_harness(tmp_path_factory.mktemp("guide"))


def input_sets():
    """score_ref's sets; set (d) without its -inf row (rows with non-finite values are not covered)"""
    return {"a": sr.set_a(), "b": sr.set_b(), "c": sr.set_c(), "d": sr.set_d()[[0, 1, 3]], "d3": sr.set_d(3)[[0, 1, 3]]}


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "d3"])
def test_harness_equals_numpy_restatement(H, name):
    """pairs (row i, row i + 1) and back, the scales in turn: S on 64 bits, max, every y[v] on 32 bits; y finite"""
    rows = input_sets()[name]
    R, V = rows.shape
    n = min(R, 6)
    lead = np.arange(n) % R
    guide = (lead + 1) % R
    guide[1::2], lead[1::2] = lead[1::2].copy(), guide[1::2].copy()      # every other pair the other way round: the guide row below the leader
    scale = np.array([SCALES[p % len(SCALES)] for p in range(n)], np.float32)
    mixed, mx, sm = gr.host_mix(H, rows, V, lead, guide, scale)
    assert np.all(np.isfinite(mixed))
    for p in range(n):
        y, ms, Ss = gr.numpy_pair(H, rows[lead[p]], rows[guide[p]], scale[p])
        assert np.array_equal(np.array(Ss).view(np.uint64), sm[p].view(np.uint64)), (name, p, "sum bits")
        assert np.array_equal(np.array(ms, np.float32), mx[p]), (name, p, "max")
        assert np.array_equal(y.view(np.uint32), mixed[p].view(np.uint32)), (name, p, "mixed bits")


def test_pinned_order_is_not_the_index_order(H):
    """on set (a) the pinned order's sum differs from the in-order chain's on at least one row (in fact on most): a kernel that sums
    in index order cannot pass as pinned. On the other sets the difference is counted, not required."""
    sets = input_sets()
    differ = {}
    for name, rows in sets.items():
        n = 0
        for x in rows:
            _, e = gr.terms(H, x)
            n += gr.pinned_sum(e) != gr.index_order_sum(e)
        differ[name] = n
    print("rows whose pinned sum differs from the index-order sum:", differ)
    assert differ["a"] >= 1
    # and the harness's sums ARE the pinned ones on set (a)
    rows = sets["a"]
    _, _, sm = gr.host_mix(H, rows, rows.shape[1], [0, 2], [1, 3], [1.5, 1.5])
    want = [[gr.pinned_sum(gr.terms(H, rows[r])[1]) for r in pair] for pair in ((0, 1), (2, 3))]
    assert np.array_equal(np.array(want).view(np.uint64), sm.view(np.uint64))


def test_short_rows_leave_partial_sums_empty(H):
    """V = 333 fills 84 of the 256 partial sums, V = 3 one: the others stay 0.0 through the butterfly"""
    for V in (333, 3, 1):
        x = (np.random.default_rng(V).standard_normal((2, V)) * 8.0).astype(np.float32)
        mixed, _, sm = gr.host_mix(H, x, V, [0], [1], [1.5])
        _, e = gr.terms(H, x[0])
        assert sm[0, 0] == gr.pinned_sum(e) and sm[0, 0] >= 1.0 and np.all(np.isfinite(mixed))
        if V <= 4:                                                  # (one group: one chain, the index order)
            assert sm[0, 0] == gr.index_order_sum(e)


def test_scale_zero_and_skipped_pairs(H):
    """scale 0 returns the guide row's log-soft-max bit for bit; a pair with lead < 0 writes nothing"""
    rows = sr.set_b()[:4]
    V = rows.shape[1]
    mixed, mx, sm = gr.host_mix(H, rows, V, [0, -1, 2], [1, 0, 3], [0.0, 1.5, 0.0], fill=-7.0)
    assert np.all(mixed[1] == -7.0) and np.all(mx[1] == -7.0) and np.all(sm[1] == -7.0)
    for p, g_row in ((0, 1), (2, 3)):
        y, _, _ = gr.numpy_pair(H, rows[g_row], rows[g_row], 1.0)      # lp_g + 1 * (lp_g - lp_g) = lp_g
        assert np.array_equal(mixed[p].view(np.uint32), y.view(np.uint32))
