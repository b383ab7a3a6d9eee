"""GPU: the instantiations of the ring-form decode launch (csrc/kernels_ring.hip) compute the same bits. The launcher picks, per shape, the
instantiation specialised for (runs of two rows, resident activation slices, a fixed number of passes per row), the DEBUG instantiation when the
phase stamps (ggml_hip_debug_stamps) or FQ_RING_DEBUG are on, and the general form for every other shape; ggml_hip_debug_ring_general(1) forces
the general form. One decode step at n_past 0 and one at n_past 5, summation orders 0 and 2: logits equal bit for bit across the three."""
import numpy as np
import pytest

import ggllm_cpp_amd as g
from oracle import binding as ob
import synth

pytestmark = pytest.mark.gpu

HP_7B_ONE_BLOCK = dict(n_vocab=512, n_embd=4544, n_head=71, n_head_kv=1, n_layer=1, n_ff=18176, two_norms=False)      # the only width that takes (R = 2, PRE, np = 3)
# four passes per row (n_embd / 32 = 200 blocks > 192): outside the specialised set, still inside the ring form's scope
HP_FOUR_PASSES = dict(n_vocab=512, n_embd=6400, n_head=100, n_head_kv=1, n_layer=1, n_ff=2048, two_norms=False)
STAMP_WORDS = 2 * 4096 * 8


@pytest.fixture(scope="module", autouse=True)
def _init():
    g.init(0)


def _weights(oracle, name):
    if name == "mqa_q4_0":
        return synth.make_model(oracle, synth.HP_TINY_MQA, ob.Q4_0, seed=21), synth.HP_TINY_MQA
    if name == "gqa_q5_1":
        return synth.make_model(oracle, synth.HP_TINY_GQA, ob.Q5_1, seed=21), synth.HP_TINY_GQA
    return synth.make_model_fast(HP_7B_ONE_BLOCK, ob.Q4_0, seed=5), HP_7B_ONE_BLOCK


def _two_steps(m, toks):
    """logits of one decode step at n_past 0 and of one at n_past 5 (behind a 5-token prompt)"""
    l0 = m.eval(toks[:1], 0).copy()
    m.eval(toks[:5], 0)
    l5 = m.eval(toks[5:6], 5).copy()
    assert m.sync_error() == 0
    return l0, l5


def _ring_stamps(L):
    """stamp rows only the ring form writes: roles 1 and 2 (epilogue wave, consumer 0) of its workgroups (every other stamping kernel stays below row 256 or
    above row 768 of the first buffer)"""
    st = np.zeros(STAMP_WORDS, np.int64)
    L.ggml_hip_debug_stamps(1, st.ctypes.data)
    return st.reshape(2, 4096, 8)[0, 256:768]


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("name", ["mqa_q4_0", "gqa_q5_1", "7b_one_block_q4_0"])
def test_plain_debug_and_general_instantiations_agree(oracle, name, mode):
    L = g.load()
    w, hp = _weights(oracle, name)
    toks = synth.tokens(6, hp["n_vocab"], seed=6)
    m = g.FalconModel(w, n_ctx=32, n_batch=8)
    m.set_fused(5)
    L.ggml_hip_reference_order(mode)
    try:
        plain = _two_steps(m, toks)
        L.ggml_hip_debug_ring_general(1)
        try:
            general = _two_steps(m, toks)
        finally:
            L.ggml_hip_debug_ring_general(0)
        L.ggml_hip_debug_stamps(1, None)
        try:
            debug = _two_steps(m, toks)
            stamped = _ring_stamps(L)
        finally:
            L.ggml_hip_debug_stamps(0, None)
    finally:
        L.ggml_hip_reference_order(0)
        m.free()
    assert (stamped != 0).any(), "the DEBUG instantiation of the ring form left no stamps"
    for step, a, b, c in zip(("n_past 0", "n_past 5"), plain, general, debug):
        assert np.array_equal(a, b), f"{step}: plain and general instantiations differ"
        assert np.array_equal(a, c), f"{step}: plain and DEBUG instantiations differ"


def test_shape_outside_the_specialised_set_takes_the_ring_form():
    """rows of four passes: the launcher has no specialised instantiation for them, launches the general ring form (its stamps show it ran) and the
    logits equal the op list's"""
    L = g.load()
    hp = HP_FOUR_PASSES
    w = synth.make_model_fast(hp, ob.Q4_0, seed=5)
    toks = synth.tokens(6, hp["n_vocab"], seed=6)
    res = {}
    for fused in (0, 5):
        m = g.FalconModel(w, n_ctx=32, n_batch=8)
        m.set_fused(fused)
        res[fused] = _two_steps(m, toks)
        if fused == 5:
            L.ggml_hip_debug_stamps(1, None)
            try:
                stamped_logits = _two_steps(m, toks)
                stamped = _ring_stamps(L)
            finally:
                L.ggml_hip_debug_stamps(0, None)
        m.free()
    assert (stamped != 0).any(), "the ring form did not run for a shape outside the specialised set"
    for a, b, c in zip(res[0], res[5], stamped_logits):
        assert np.array_equal(a, b)
        assert np.array_equal(a, c)
