"""CPU: the yardstick of the F16 mat-mul tests (tests/f16_ref.py) against the real reference's scalar build, and the teeth of its
adversarial inputs: on the cancelling rows every other association of the same terms gives other f32 bits."""
import numpy as np
import pytest

import f16_ref
from oracle import binding as ob

SHAPES = [(96, 65, 3), (4544, 130, 2), (18176, 40, 1)]


@pytest.mark.skipif(not ob.Ref.available(scalar=True), reason="oracle/_ref/libggml_ref_scalar.so is not built")
@pytest.mark.parametrize("gen", list(f16_ref.GENERATORS))
@pytest.mark.parametrize("K,M,N", SHAPES)
def test_yardstick_is_the_reference_scalar_build(gen, K, M, N):
    ref = ob.Ref(scalar=True)
    w, x, y = f16_ref.case(gen, K, M, N)
    for threads in (1, 3, 4):
        got = ref.mul_mat(1, w.view(np.uint8), K, M, x, n_threads=threads)
        assert np.array_equal(f16_ref.bits(got), f16_ref.bits(y)), (gen, K, M, N, threads)


@pytest.mark.parametrize("K", [96, 256, 4544])
def test_cancelling_rows_have_teeth(K):
    M = 130
    w, x, y = f16_ref.case("cancelling_rows", K, M, 2)
    for n in range(2):
        t = f16_ref.terms(w, x[n])
        assert np.array_equal(f16_ref.bits(f16_ref.order_sequential(t)), f16_ref.bits(y[n]))
        for name, fn in (("reversed", f16_ref.order_reversed), ("groups of 8", f16_ref.order_groups_of_8), ("64 strided lanes", f16_ref.order_strided_lanes)):
            differ = np.mean(f16_ref.bits(fn(t)) != f16_ref.bits(y[n]))
            assert differ >= 0.9, (K, name, differ)


def test_edge_values_round_as_the_contract_says():
    # token 0 of the model-like inputs: subnormal fp16 results, a tie (1 + 2^-11 -> 1, to even), the largest fp16
    x16 = f16_ref.EDGE.astype(np.float16)
    assert x16[3] == np.float16(5.96e-8) and x16[3].view(np.uint16) == 1          # the smallest subnormal
    assert x16[4] == 0 and x16[6] == 1 and x16[7] == np.float16(65504)
    assert np.isfinite(x16.astype(np.float32)).all()
