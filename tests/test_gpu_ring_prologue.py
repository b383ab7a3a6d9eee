"""GPU: the helpers' prologue of the ring-form decode launch (csrc/kernels_ring.hip: every helper thread loads its float4 quads of the residual row
itself and keeps them in registers -- two up to n_embd 5632, three beyond --, LayerNorm statistics, Q8 image) at the widths where the dealing of the
row to the 704 helper threads can go wrong. The ring form (fused mode 5) must give the logits and hidden states of the register-streaming launch
(mode 1) and of the op list (mode 0), bit for bit, in the default order and in the fast reference order, specialised and general instantiation alike.

n_embd   quads   what it exercises
   64      16    a quarter of one wave, ten waves with nothing
 2048     512    SPEC = 1, three idle waves, no second quad anywhere
 4544    1136    the real width: every thread one quad, 432 threads a second one
 5632    1408    exactly two quads per thread: the last width of the two-quad form
 5696    1424    the first thread with a third quad
 8448    2112    the largest width in scope: three quads for every thread
 4608    1152    two norms: the second image from the kept (x - mean) * scale
"""
import numpy as np
import pytest

import ggllm_cpp_amd as g
from oracle import binding as ob
import synth

gpu = pytest.mark.gpu

WIDTHS = [64, 2048, 4544, 5632, 5696, 8448]
N_FF = 1024
CASES = [(E, ob.Q4_0, False, False) for E in WIDTHS] + [(4608, ob.Q4_0, True, False)] \
      + [(E, t, False, False) for t in (ob.Q5_1, ob.Q8_0) for E in (64, 4544, 5696)] \
      + [(4544, ob.Q4_0, False, True)]                                # (the last: every launch through the general instantiation)


def _hp(E, two):
    return dict(n_vocab=512, n_embd=E, n_head=E // 64, n_head_kv=2 if two else 1, n_layer=1, n_ff=N_FF, two_norms=two)


def test_every_width_is_in_the_ring_launchers_scope():
    """fq_launch_gemv_ln_ring launches nothing (and the caller falls back to k_gemv_ln) outside n_embd % 32 == 0, n_embd <= 8448, n_ff % 32 == 0 and at most
    twelve 32-row groups of Wup per workgroup: a width outside would make the GPU test compare k_gemv_ln with itself"""
    assert len(CASES) == 14
    for E, _t, two, _general in CASES:
        hp = _hp(E, two)
        assert E % 64 == 0 and hp["n_head"] * 64 == E
        assert E % 32 == 0 and E <= 8448 and hp["n_ff"] % 32 == 0
        assert hp["n_ff"] <= 32 * 12 * 8                              # (a grid of 8 workgroups would do; an MI355X has 256)
    assert {E for E, t, _two, _g in CASES if t == ob.Q4_0} == set(WIDTHS) | {4608}
    assert 2 * 704 * 4 == 5632 and 5696 // 4 == 2 * 704 + 16 and 8448 // 4 == 3 * 704      # the two-quad form ends where the table says it does


@pytest.fixture(scope="module")
def _init():
    g.init(0)


def _steps(w, toks, order, mode, general):
    L = g.load()
    m = g.FalconModel(w, n_ctx=32, n_batch=4)
    m.set_fused(mode)
    L.ggml_hip_reference_order(order)
    L.ggml_hip_debug_ring_general(1 if general else 0)
    try:
        m.eval(toks[:4], 0)
        r = [m.eval(toks[i:i + 1], i, want_hidden=True) for i in range(4, 10)]
        assert m.sync_error() == 0
    finally:
        L.ggml_hip_debug_ring_general(0)
        L.ggml_hip_reference_order(0)
        m.free()
    return r


@gpu
@pytest.mark.parametrize("E,t,two,general", CASES, ids=[f"{E}-t{t}{'-2n' if two else ''}{'-general' if gen else ''}" for E, t, two, gen in CASES])
def test_ring_prologue_bit_identical_to_the_other_forms(_init, E, t, two, general):
    w = synth.make_model_fast(_hp(E, two), t, seed=31)
    toks = synth.tokens(10, 512, seed=13)
    for order in (0, 2):
        ring = _steps(w, toks, order, 5, general)
        for mode in (1, 0):
            other = _steps(w, toks, order, mode, False)
            for i, ((la, ha), (lb, hb)) in enumerate(zip(ring, other)):
                assert np.array_equal(ha, hb), f"order {order}, step {i}: hidden states differ from fused mode {mode}"
                assert np.array_equal(la, lb), f"order {order}, step {i}: logits differ from fused mode {mode}"
