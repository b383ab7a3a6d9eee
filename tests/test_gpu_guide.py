"""GPU: the guidance mix on the device. ggml_hip_guide_rows (csrc/kernels_guide.hip) against the host statement of the same header
(tests/host/guide_harness.cpp, itself pinned to an independent numpy restatement by tests/test_guide_cpu.py): the 64 bits of the two
double sums in the pinned order, the maxima and the 32 bits of every mixed value; every output starts as a sentinel."""
import numpy as np
import pytest

import ggllm_cpp_amd as g
import guide_ref as gr
import score_ref as sr

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
GAP = 1e30
SCALES = [1.5, 1.0, 0.0, -0.5, 7.5]


@pytest.fixture(scope="module")
def L():
    L = g.load()
    L.ggml_hip_init(0)
    return L


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return gr.build_harness(tmp_path_factory.mktemp("guide"))


def base_rows(V, seed=0):
    """6 rows of V logits: two N(0, 8^2), two uniform over [-120, 0] (terms go denormal and zero, lp must not), the maximum at index 0, at V - 1"""
    rng = np.random.default_rng(1000 + V + seed)
    x = np.empty((6, V), np.float32)
    x[0:2] = (rng.standard_normal((2, V)) * 8.0).astype(np.float32)
    x[2:4] = rng.uniform(-120.0, 0.0, (2, V)).astype(np.float32)
    x[4:6] = (rng.standard_normal((2, V)) * 8.0).astype(np.float32)
    x[4, 0] = x[4].max() + 1.0
    x[5, V - 1] = x[5].max() + 1.0
    return x


def device_mix(L, rows, V, lead, guide, scale, mixed_stride=None, want_stats=True):
    """one launch over rows [R][stride]; mixed [P][mixed_stride], max [P][2], sum [P][2], all SENTINEL before; the logits as the launch left them"""
    R, S = rows.shape
    P = len(lead)
    ms = V if mixed_stride is None else mixed_stride
    lg = g.DevBuf(host=rows)
    ld, gd = g.DevBuf(host=np.ascontiguousarray(lead, np.int32)), g.DevBuf(host=np.ascontiguousarray(guide, np.int32))
    sc = g.DevBuf(host=np.ascontiguousarray(scale, np.float32))
    mx, mb, sb = g.DevBuf(host=np.full((P, ms), SENTINEL, np.float32)), g.DevBuf(host=np.full((P, 2), SENTINEL, np.float32)), g.DevBuf(host=np.full((P, 2), SENTINEL, np.float64))
    try:
        g.guide_rows(lg, S, V, P, ld, gd, sc, mx, ms, mb if want_stats else None, sb if want_stats else None)
        L.ggml_hip_synchronize()
        return mx.to_host(np.float32, (P, ms)), mb.to_host(np.float32, (P, 2)), sb.to_host(np.float64, (P, 2)), lg.to_host(np.float32, (R, S))
    finally:
        for b in (lg, ld, gd, sc, mx, mb, sb):
            b.free()


def check_launch(L, H, rows, V, lead, guide, scale, mixed_stride=None):
    lead, guide = np.asarray(lead), np.asarray(guide)
    want_y, want_m, want_s = gr.host_mix(H, rows, V, lead, guide, scale, fill=SENTINEL)
    got_y, got_m, got_s, after = device_mix(L, rows, V, lead, guide, scale, mixed_stride)
    on = lead >= 0
    assert on.any() and np.all(np.isfinite(want_y[on]))
    assert np.array_equal(after.view(np.uint32), np.ascontiguousarray(rows, np.float32).view(np.uint32)), "the logits were written"
    assert np.array_equal(got_s[on].view(np.uint64), want_s[on].view(np.uint64)), "sum bits"
    assert np.array_equal(got_m[on], want_m[on]) and np.all(got_m[on] < 1e29), "max"
    assert np.array_equal(got_y[:, :V][on].view(np.uint32), want_y[on].view(np.uint32)), "mixed bits"
    assert np.all(got_y[:, V:] == SENTINEL), "written beyond n_vocab"
    assert np.all(got_y[~on] == SENTINEL) and np.all(got_m[~on] == SENTINEL) and np.all(got_s[~on] == SENTINEL), "an absent pair's slots were written"
    return got_y, got_m, got_s


def padded(x, pad):
    """rows pad floats apart beyond V, the gap filled with 1e30: it must not be read"""
    out = np.full((x.shape[0], x.shape[1] + pad), GAP, np.float32)
    out[:, :x.shape[1]] = x
    return out


# V: Falcon's vocabulary; 4099: no multiple of 4 -- element-wise loads, unaligned rows; 333: fewer groups than lanes (some q_j stay 0.0); 3: one group
@pytest.mark.parametrize("pad", [0, 7])
@pytest.mark.parametrize("V", [65024, 4099, 333, 3])
def test_kernel_matches_harness(L, H, V, pad):
    """three pairs in one launch with three scales: the guide row above its leader, below it, and a pair of the wide-range rows; a pair
    slot that is absent keeps its sentinels, the row no pair names stays as it is; row_stride = V + 7 puts 1e30 between the rows"""
    rows = padded(base_rows(V), pad)
    lead, guide = [0, 5, -1, 2], [1, 4, 0, 3]
    check_launch(L, H, rows, V, lead, guide, [1.5, -0.5, 1.0, 7.5], mixed_stride=V + (5 if pad else 0))


@pytest.mark.parametrize("V", [65024, 333])
def test_every_scale_and_two_pairs(L, H, V):
    rows = base_rows(V, seed=1)
    for i in range(0, len(SCALES), 2):
        sc = (SCALES + SCALES)[i:i + 2]
        check_launch(L, H, rows, V, [3, 0], [2, 4], sc)


def test_pair_alone_and_third_of_three(L, H):
    """the same pair gives the same bits alone in a launch and as the third of three"""
    V = 65024
    rows = base_rows(V, seed=2)
    a = check_launch(L, H, rows, V, [1], [4], [1.5])
    b = check_launch(L, H, rows, V, [0, 2, 1], [5, 3, 4], [7.5, 0.0, 1.5])
    assert np.array_equal(a[0][0].view(np.uint32), b[0][2].view(np.uint32)) and np.array_equal(a[2][0].view(np.uint64), b[2][2].view(np.uint64))


def test_sums_are_the_pinned_order_not_the_index_order(L, H):
    """on score_ref's set (a) the device's sums are the pinned order's and differ from the index-order chain's (ggml_hip_score_rows') on at least one row"""
    rows = sr.set_a()[:6]
    V = rows.shape[1]
    _, _, got_s = check_launch(L, H, rows, V, [0, 2, 4], [1, 3, 5], [1.5, 1.5, 1.5])
    chain = np.array([[gr.index_order_sum(gr.terms(H, rows[r])[1]) for r in pair] for pair in ((0, 1), (2, 3), (4, 5))])
    assert np.any(got_s != chain)


def test_kernel_ignores_reference_order_and_optional_outputs(L, H):
    V = 4099
    rows = base_rows(V, seed=3)
    L.ggml_hip_reference_order(2)
    try:
        check_launch(L, H, rows, V, [0, 3], [1, 2], [1.5, -0.5])
    finally:
        L.ggml_hip_reference_order(0)
    want_y, _, _ = gr.host_mix(H, rows, V, [0], [1], [1.5])
    got_y, got_m, got_s, _ = device_mix(L, rows, V, [0], [1], [1.5], want_stats=False)
    assert np.array_equal(got_y.view(np.uint32), want_y.view(np.uint32)) and np.all(got_m == SENTINEL) and np.all(got_s == SENTINEL)
