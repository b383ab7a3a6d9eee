"""CPU: the oracle at the extremes of the block encodings (tests/extreme_blocks.py: negative, zero and subnormal d / dmin, saturated planes and
scales, saturated and cancelling activation rows) against the recorded results of both reference builds (tests/golden/extreme_blocks.npz), on
the BIT PATTERNS: -0.0 and +0.0 are different answers here. The GPU side is tests/test_gpu_extreme_blocks.py; the kernels' unit arithmetic on
the same blocks, host-compiled, is in tests/test_units_host.py."""
import numpy as np
import pytest

from oracle import binding as ob
import extreme_blocks as xb
import extreme_host as xh

CASES = list(xb.cases())
IDS = [c[0] for c in CASES]


@pytest.fixture(scope="module")
def quantize(oracle):
    return xh.cpu_quantizer(oracle)


@pytest.fixture(scope="module")
def order0(oracle, quantize):
    """name -> (w, oracle order-0 outputs [16, M]), computed once"""
    out = {}
    for name, t, fam, K, M in CASES:
        w = xh.case_weights(name, t, fam, K, quantize, M)
        out[name] = (w, xh.oracle_mul_mat(oracle, 0, t, w, K, xh.activations(K)))
    return out


def test_fixture_holds_every_case():
    g = xh.golden()
    assert len(CASES) == 105
    for name, t, fam, K, M in CASES:
        assert g[f"{name}_y_scalar"].shape == g[f"{name}_y_avx"].shape == (16, M)
        assert g[f"{name}_err"].shape == (2,) and 0 < g[f"{name}_err"].max() < 1e-4      # in units of sum |w| |x|: f32 association, no more
        assert (f"{name}_deq" in g) == fam.startswith("saturated")
        # neither reference build ever answers -0.0, not even for rows of d = dmin = -0
        assert not (xh.bits(g[f"{name}_y_scalar"]) == xh.NEG_ZERO).any() and not (xh.bits(g[f"{name}_y_avx"]) == xh.NEG_ZERO).any()


@pytest.mark.parametrize("name,t,fam,K,M", CASES, ids=IDS)
def test_order0_is_the_scalar_build_bit_for_bit(oracle, order0, name, t, fam, K, M):
    w, y = order0[name]
    assert np.array_equal(xh.bits(y), xh.bits(xh.golden()[f"{name}_y_scalar"]))
    if ob.Ref.available(scalar=True):
        live = ob.Ref(scalar=True).mul_mat(t, w, K, w.shape[0], xh.activations(K), 2)
        assert np.array_equal(xh.bits(y), xh.bits(live))


@pytest.mark.parametrize("name,t,fam,K,M", [c for c in CASES if c[2].startswith("saturated")], ids=[c[0] for c in CASES if c[2].startswith("saturated")])
def test_dequantize_equals_the_recorded_rows(oracle, order0, name, t, fam, K, M):
    w, _ = order0[name]
    rows = range(w.shape[0]) if K <= 256 else xb.DEQ_ROWS_LONG
    got = np.stack([oracle.dequantize(t, w[r], K) for r in rows])
    assert np.array_equal(xh.bits(got), xh.bits(xh.golden()[f"{name}_deq"]))
    assert np.abs(got).max() > 0


@pytest.mark.parametrize("order", [2, 3, 4, 5])
@pytest.mark.parametrize("name,t,fam,K,M", CASES, ids=IDS)
def test_backend_orders_keep_the_sign_of_zero_and_the_bound(oracle, order0, name, t, fam, K, M, order):
    """the oracle's restatements of the kernels' associations: no -0.0 where the reference answers +0.0 (it never answers -0.0), and the same terms --
    within the case's term-magnitude bound of the f64 product"""
    w, _ = order0[name]
    x = xh.activations(K)
    wv = np.stack([oracle.dequantize(t, w[r], K) for r in range(w.shape[0])])
    av = xb.act_values(ob.VEC_DOT[t], xh.act_image(oracle, t, x), K)
    for N in (4, 16):                                                   # mode 2 picks its order by the batch: the mat-vec kernels' and the GEMMs'
        y = xh.oracle_mul_mat(oracle, order, t, w, K, x[:N])
        assert not (xh.bits(y) == xh.NEG_ZERO).any()
        assert xb.term_error(y, wv, av[:N]) <= xh.bound(name)


@pytest.mark.parametrize("name,t,fam,K,M", CASES, ids=IDS)
def test_cases_are_not_vacuous(order0, name, t, fam, K, M):
    """outside the all-zero activation row and the weight rows whose every d is +-0, at most 2 % of a case's expected outputs are exactly zero"""
    w, y = order0[name]
    live = y[np.arange(16) != xh.ZERO_ROW][:, ~xb.dead_rows(w, t)]
    assert live.size >= 15 * 25
    assert (live == 0).sum() <= 0.02 * live.size, (int((live == 0).sum()), live.size)
    assert not y[xh.ZERO_ROW].any() and not y[:, xb.dead_rows(w, t)].any()
