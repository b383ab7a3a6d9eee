"""GPU: every mat-mul form at the extremes of the block encodings (tests/extreme_blocks.py): negative, zero and subnormal d / dmin, saturated
planes with every sub-block scale and min at its extreme, rows the weight quantizer writes (both signs of d in Q3_K / Q6_K), against saturated,
cancelling, sparse, zero, huge and tiny activation rows. Each form == the oracle in the order that form is paired with elsewhere in the suite, on
the uint32 VIEWS (a -0.0 where the reference answers +0.0 is a deviation), the reference orders == the recorded scalar build
(tests/golden/extreme_blocks.npz), and every result within the case's recorded term-magnitude bound of the f64 product.
Arithmetic: ggml_vec_dot_q*_q8_* (ggml.c:2397-3330), ggml_vec_dot_q*_K_q8_K (k_quants.c:1267-2789), the quantizers' d = 1 / (-32 / max_scale)
and 1 / (-128 / max_scale) (restated in csrc/fq_wquant.h), quantize_row_q8_K_reference (k_quants.c:899-934)."""
import numpy as np
import pytest

import ggllm_cpp_amd as g
from oracle import binding as ob
import extreme_blocks as xb
import extreme_host as xh
import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _init():
    g.init(0)
    # the launchers latch "no FQ_GEMM_CFG in the environment" at their first call: make that call here, before any test of this file sets it
    rng = np.random.default_rng(1)
    for t in ob.WEIGHT_TYPES:
        dw = g.Weight(t, synth.random_blocks(t, 8, 512, rng), 512, 8)
        for N in (5, 17, 33):
            dw.mul_mat(rng.standard_normal((N, 512)).astype(np.float32))
        dw.free()


def device_quantize(t, x):
    return g.quantize_rows(t, x)          # pinned to the reference's vectors by tests/test_gpu_wquant.py; the recorded sha256 pins it here again


class switch:
    """one of the library's process-wide test switches, put back on exit"""

    def __init__(self, name, value):
        self.fn, self.value = getattr(g.load(), name), value

    def __enter__(self):
        self.fn(self.value)

    def __exit__(self, *exc):
        self.fn(0)


def run_forms(dw, A, legacy, monkeypatch):
    """(form, N, oracle order) -> device result, default forms first"""
    out = {}
    for N in (1, 4, 5, 16, 17, 33):       # mat-vec | streaming | streaming, two passes | tile GEMM
        out["default", N, 2] = dw.mul_mat(xb.rows_for(A, N))
    with switch("ggml_hip_gemm_sequential", 1):
        for N in (5, 16, 17, 33):
            out["sequential", N, 5] = dw.mul_mat(xb.rows_for(A, N))
    for mode in (1, 2):
        with switch("ggml_hip_reference_order", mode):
            for N in (1, 4):
                out[f"reference{mode}", N, 0] = dw.mul_mat(xb.rows_for(A, N))
    with switch("ggml_hip_debug_force_gemv", 1):
        out["forced_gemv", 33, 1] = dw.mul_mat(xb.rows_for(A, 33))
    for cfg, order in ((6, 4), (7, 3)):   # the 64-row workgroups <2,4,2> and <4,4,2> (the latter is not used for k-quants: register budget)
        if cfg == 7 and not legacy:
            continue
        monkeypatch.setenv("FQ_GEMM_CFG", str(cfg))
        try:
            out[f"cfg{cfg}", 33, order] = dw.mul_mat(xb.rows_for(A, 33))
        finally:
            monkeypatch.delenv("FQ_GEMM_CFG")
    return out


@pytest.mark.parametrize("fam", xb.FAMILIES)
@pytest.mark.parametrize("t", ob.WEIGHT_TYPES)
def test_every_form_at_the_extremes(oracle, monkeypatch, t, fam):
    """Measured on the MI355X: every form bit-identical with its oracle order; the device's term-magnitude errors are listed in NOTEBOOK.md next
    to the reference's recorded ones."""
    gold = xh.golden()
    for name, _, _, K, M in xb.cases_of(t, fam):
        w = xh.case_weights(name, t, fam, K, device_quantize, M)      # `quantizer`: real blocks, quantized on the device
        A = xh.activations(K)
        dw = g.Weight(t, w, K, M)
        try:
            got = run_forms(dw, A, t in ob.LEGACY, monkeypatch)
            deq = dw.dequantize()
        finally:
            dw.free()
        wv = np.stack([oracle.dequantize(t, w[r], K) for r in range(M)])
        assert np.array_equal(xh.bits(deq), xh.bits(wv))
        av = xb.act_values(ob.VEC_DOT[t], xh.act_image(oracle, t, A), K)
        y_scalar = gold[f"{name}_y_scalar"]
        worst, bad = 0.0, []
        for (form, N, order), y in got.items():
            exp = xh.oracle_mul_mat(oracle, order, t, w, K, xb.rows_for(A, N))
            e = xb.term_error(y, wv, xb.rows_for(av, N))
            worst = max(worst, e)
            print(f"EXTREME {name} {form} N={N} term_error {e:.3e} (reference builds {gold[name + '_err'][0]:.3e} {gold[name + '_err'][1]:.3e})")
            if not np.array_equal(xh.bits(y), xh.bits(exp)):
                diff = xh.bits(y) != xh.bits(exp)
                bad.append((form, N, f"!= oracle order {order}", int(diff.sum()), int((xh.bits(y)[diff] == xh.NEG_ZERO).sum())))
            if order == 0 and not np.array_equal(xh.bits(y), xh.bits(xb.rows_for(y_scalar, N))):
                bad.append((form, N, "!= recorded y_scalar"))
            if e > xh.bound(name):
                bad.append((form, N, "term error", e, xh.bound(name)))
        print(f"EXTREME_WORST {name} device {worst:.3e} scalar {gold[name + '_err'][0]:.3e} avx {gold[name + '_err'][1]:.3e}")
        assert not bad, (name, bad)


@pytest.mark.parametrize("hi", [False, True])
@pytest.mark.parametrize("t", ob.WEIGHT_TYPES)
def test_dequantize_rows_equal_the_recorded_rows(t, hi):
    """Weight.dequantize() (ggml_hip_dequantize_rows) on the saturated planes: all rows, and repeated / arbitrary row indices, bit for bit"""
    fam = "saturated_hi" if hi else "saturated_lo"
    for name, _, _, K, M in xb.cases_of(t, fam):
        w = xh.case_weights(name, t, fam, K, None, M)
        rec = xh.golden()[f"{name}_deq"]
        rec_rows = list(range(w.shape[0])) if K <= 256 else list(xb.DEQ_ROWS_LONG)
        dw = g.Weight(t, w, K, w.shape[0])
        try:
            full = dw.dequantize()
            pick = [36, 0, 0, 17, 1, 36, 17]
            some = dw.dequantize(rows=pick)
        finally:
            dw.free()
        assert np.array_equal(xh.bits(full[rec_rows]), xh.bits(rec))
        assert np.array_equal(xh.bits(some), xh.bits(full[pick]))
        assert np.abs(full).min(axis=1).max() > 0                     # saturated: some row has no zero weight at all


@pytest.mark.parametrize("act_t,K", [(a, K) for a in (ob.Q8_0, ob.Q8_1, ob.Q8_K) for K in (64, 256, 2304, 4096, 4544) if K % ob.BLCK[a] == 0])
def test_activation_images_equal_the_oracle(oracle, act_t, K):
    """g.quantize_acts on the saturated, cancelling, sparse, zero, huge and tiny rows == the oracle's image, byte for byte (Q8_0 / Q8_1 scales
    that are fp16 subnormals, Q8_K rows of -128 with bsums of -2048)"""
    A = xh.activations(K)
    got = g.quantize_acts(act_t, A)
    exp = np.stack([oracle.quantize_act(act_t, row) for row in A])
    assert np.array_equal(got, exp)


# ---------------------------------------------------------------------------------------------------------------- the decode launches
def _model(t, fam, seed):
    """one decoder block whose every matrix comes from `fam`: the k-quants at 4096 (the narrowest width that is whole unit columns for all of them:
    fq_lay<TYPE>::CB = 16 super-blocks for Q2_K / Q3_K, 8 for Q4_K .. Q6_K), the legacy formats at Falcon-7B's 4544"""
    if t in ob.KQUANTS:
        hp = dict(n_vocab=512, n_embd=4096, n_head=64, n_head_kv=8, n_layer=1, n_ff=16384, two_norms=True)
    else:
        hp = dict(n_vocab=512, n_embd=4544, n_head=71, n_head_kv=1, n_layer=1, n_ff=18176, two_norms=False)
    E, H, HKV, FF, V = hp["n_embd"], hp["n_head"], hp["n_head_kv"], hp["n_ff"], hp["n_vocab"]
    idx = [0]

    def mat(rows, k):
        idx[0] += 1
        if fam == "quantizer":            # ordinary weights through the device's quantizer: Q3_K / Q6_K blocks of both signs of d
            x = (np.random.default_rng([seed, idx[0]]).standard_normal((rows, k)) * 0.02).astype(np.float32)
            w = g.quantize_rows(t, x)
            if t in (ob.Q3_K, ob.Q6_K):
                d = xb.get_h(w, t, 0)
                assert 4 * xb.h_is_negative(d).sum() >= d.size and 4 * (~xb.h_is_negative(d)).sum() >= d.size
            return w
        return xb.weights(t, "signed_d", rows, k, seed + idx[0], values=xb.D_VALUES_NO_TWO)

    def ln():
        idx[0] += 1
        r = np.random.default_rng([seed, idx[0]])
        return ((1.0 + 0.02 * r.standard_normal(E)).astype(np.float32), (0.02 * r.standard_normal(E)).astype(np.float32))

    m = dict(hparams=hp, wtype=t, layers=[])
    m["tok_emb"] = mat(V, E)
    lw = dict(qkv=mat((H + 2 * HKV) * 64, E), wo=mat(E, E), up=mat(FF, E), down=mat(E, FF))
    lw["ln_w"], lw["ln_b"] = ln()
    if hp["two_norms"]:
        lw["ln2_w"], lw["ln2_b"] = ln()
    m["layers"].append(lw)
    m["out_norm_w"], m["out_norm_b"] = ln()
    m["lm_head"] = mat(V, E)
    return m


@pytest.mark.parametrize("fam", ["signed_d", "quantizer"])
@pytest.mark.parametrize("t", ob.KQUANTS + [ob.Q4_0, ob.Q5_1])
def test_decode_launches_at_the_extremes(oracle, t, fam):
    """3-token prompt + 3 decode steps: the op list (0), the register-streaming launches (1) and the ring forms (5) give the same logits and hidden
    states on the uint32 views, and they are the oracle model's in backend order"""
    w = _model(t, fam, 77)
    hp = w["hparams"]
    toks = synth.tokens(6, hp["n_vocab"], seed=4)
    outs = []
    for mode in (0, 1, 5):
        m = g.FalconModel(w, n_ctx=16, n_batch=4)
        try:
            m.set_fused(mode)
            m.eval(toks[:3], 0)
            outs.append([m.eval(toks[i:i + 1], i, want_hidden=True) for i in range(3, 6)])
            assert m.sync_error() == 0
        finally:
            m.free()
    for lg, hid in outs[0]:
        assert np.isfinite(lg).all() and np.isfinite(hid).all() and np.abs(lg).max() > 0
    for other in outs[1:]:
        for (la, ha), (lb, hb) in zip(outs[0], other):
            assert np.array_equal(xh.bits(ha), xh.bits(hb))
            assert np.array_equal(xh.bits(la), xh.bits(lb))
    oracle.lib.orc_set_sum_order(2)
    try:
        mo = oracle.model(w, 16)
        mo.eval(toks[:3], 0, 16)
        want = [mo.eval(toks[i:i + 1], i, 16)[0] for i in range(3, 6)]
    finally:
        oracle.lib.orc_set_sum_order(0)
    for (lg, _), b in zip(outs[0], want):
        assert np.array_equal(xh.bits(lg[0]), xh.bits(b))
