"""GPU parity: layer norm, GELU, RoPE + KV append, attention -- against the oracle and the golden vectors."""
import ctypes

import numpy as np
import pytest

import ggllm_cpp_amd as g
from oracle import binding as ob
from decode_attn import attention_ref as _attention_ref      # the plain numpy f64 attention, shared with test_gpu_decode_attention.py

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _init():
    g.init(0)


def relrms(a, b):
    return float(np.abs(a.astype(np.float64) - b).max() / (np.sqrt((b.astype(np.float64) ** 2).mean()) + 1e-30))


def test_wave_reductions_selftest():
    """DPP / readlane wave reductions == plain __shfl_xor butterfly, bit for bit (f32, f64, i32 sums and f32 max)"""
    assert g.load().ggml_hip_selftest() == 0


def test_exp_formula_reproduces_table():
    """the in-kernel recomputation of soft_max's EXP table entry (fp16(exp(fp32(h))) through f64) equals the host-built
    table for every non-NaN fp16 input -- the condition under which the attention kernels use it instead of a gather"""
    assert g.load().ggml_hip_exp_formula_mismatches() == 0


def test_tables_match_reference(oracle, golden):
    """the fp16 GELU / EXP tables the kernels index are the reference's (ggml.c:4276-4290), bit for bit"""
    L = g.load()
    gelu = np.empty(1 << 16, np.uint16)
    ex = np.empty(1 << 16, np.uint16)
    L.ggml_hip_memcpy_d2h(gelu.ctypes.data, L.ggml_hip_gelu_table_dev(), 1 << 17)
    L.ggml_hip_memcpy_d2h(ex.ctypes.data, L.ggml_hip_exp_table_dev(), 1 << 17)
    gb = golden["block_ops"]
    assert np.array_equal(gelu[gb["gelu_all_in_bits"]], gb["gelu_all_out_bits"])
    fin = np.isfinite(np.arange(1 << 16, dtype=np.uint16).view(np.float16).astype(np.float32))
    assert np.array_equal(gelu[fin], oracle.gelu_table()[fin])
    assert np.array_equal(ex[fin], oracle.exp_table()[fin])


@pytest.mark.parametrize("n,rows", [(4544, 5), (8192, 3), (256, 9)])
def test_layer_norm(oracle, golden, n, rows):
    L = g.load()
    rng = np.random.default_rng(n)
    x = (rng.standard_normal((rows, n)) * 3 + 0.5).astype(np.float32)
    if n == 4544:
        x = golden["block_ops"]["norm_x"]
    w = (1 + 0.02 * rng.standard_normal(n)).astype(np.float32)
    b = (0.02 * rng.standard_normal(n)).astype(np.float32)
    xb, wb, bb, yb = g.DevBuf(host=x), g.DevBuf(host=w), g.DevBuf(host=b), g.DevBuf(x.nbytes)
    L.ggml_hip_layer_norm(xb.ptr, n, rows, None, None, yb.ptr)
    plain = yb.to_host(np.float32, x.shape)
    L.ggml_hip_layer_norm(xb.ptr, n, rows, wb.ptr, bb.ptr, yb.ptr)
    full = yb.to_host(np.float32, x.shape)
    # f64 sums: only their association differs from the reference -> equal up to 1 ulp of the f32 mean/variance
    assert relrms(plain, oracle.norm(x)) <= 1e-6
    assert relrms(full, oracle.layer_norm(x, w, b)) <= 1e-6
    if n == 4544:
        assert relrms(plain, golden["block_ops"]["norm_y"]) <= 1e-6
    print("layer_norm bit-identical elements:", float((plain == oracle.norm(x)).mean()))


def test_gelu_bit_exact(oracle, golden):
    L = g.load()
    gb = golden["block_ops"]
    x = gb["gelu_x"]
    xb, yb = g.DevBuf(host=x), g.DevBuf(x.nbytes)
    L.ggml_hip_gelu(xb.ptr, yb.ptr, x.size)
    assert np.array_equal(yb.to_host(np.float32, x.shape), gb["gelu_y"])


@pytest.mark.parametrize("n_ctx", [2048, 8192])
def test_rope_kv_store(oracle, golden, n_ctx):
    L = g.load()
    gb = golden["block_ops"]
    N, H, HKV, D, n_past = 3, 4, 1, 64, 1021
    x = gb[f"rope_x_{n_ctx}"]                    # [3, 5, 64] = per token: 4 q heads + 1 k head
    rng = np.random.default_rng(1)
    v = rng.standard_normal((N, HKV, D)).astype(np.float32)
    qkv = np.concatenate([x, v], axis=1)         # [N, H + 2*HKV, D]
    tab = L.ggml_hip_rope_table_create(D, n_past + N, n_ctx)
    qb = g.DevBuf(host=qkv)
    kc, vc = g.DevBuf((n_past + N) * HKV * D * 4), g.DevBuf((n_past + N) * HKV * D * 4)
    L.ggml_hip_rope_kv_store(qb.ptr, N, H, HKV, D, n_past, tab, kc.ptr, vc.ptr)
    out = qb.to_host(np.float32, qkv.shape)
    ref = gb[f"rope_y_{n_ctx}"]
    assert np.array_equal(out[:, :H], ref[:, :H])                       # Q rotated in place
    kcache = kc.to_host(np.float32, (n_past + N, HKV, D))
    vcache = vc.to_host(np.float32, (n_past + N, HKV, D))
    assert np.array_equal(kcache[n_past:], ref[:, H:H + HKV])           # K rotated into the cache
    assert np.array_equal(vcache[n_past:], v)
    assert np.array_equal(out[:, H:], qkv[:, H:])                       # K/V slots of the fused row untouched
    assert np.array_equal(ref, oracle.rope(x, 64, 5, 3, n_past, n_ctx))


# (the last three: the prefill kernel's other shapes -- 2 tokens per workgroup beyond ~3000 keys, one token per workgroup
#  when two score rows no longer fit LDS, and a ragged last token block; then the shapes that are re-routed at long contexts -- batches of 4 .. 31 tokens
#  beyond 3000 keys, and the f64 variant with N >= 32)
@pytest.mark.parametrize("H,HKV,N,n_past", [(4, 1, 1, 0), (71, 1, 1, 300), (8, 2, 5, 37), (16, 8, 3, 1000), (2, 1, 6, 3500),
                                            (2, 1, 2, 20000), (3, 1, 7, 0), (2, 1, 16, 3500), (3, 1, 31, 5000), (8, 2, 4, 3100), (2, 1, 40, 3000)])
def test_attention(oracle, H, HKV, N, n_past):
    L = g.load()
    D = 64
    rng = np.random.default_rng(H * 100 + N)
    n_kv = n_past + N
    qkv = rng.standard_normal((N, H + 2 * HKV, D)).astype(np.float32)
    kc = rng.standard_normal((n_kv, HKV, D)).astype(np.float32)
    vc = rng.standard_normal((n_kv, HKV, D)).astype(np.float32)
    qb, kb, vb, ob_ = g.DevBuf(host=qkv), g.DevBuf(host=kc), g.DevBuf(host=vc), g.DevBuf(N * H * D * 4)
    L.ggml_hip_attention(qb.ptr, N, H, HKV, D, n_past, kb.ptr, vb.ptr, ob_.ptr)
    got = ob_.to_host(np.float32, (N, H * D))
    L.ggml_hip_reference_order(1)            # f64 accumulation of the two dot products, like the reference's portable build
    try:
        L.ggml_hip_attention(qb.ptr, N, H, HKV, D, n_past, kb.ptr, vb.ptr, ob_.ptr)
        got64 = ob_.to_host(np.float32, (N, H * D))
    finally:
        L.ggml_hip_reference_order(0)
    exp = _attention_ref(oracle, qkv[:, :H], kc, vc, n_past, H, HKV)
    assert relrms(got64, exp) <= 2e-6, relrms(got64, exp)
    # default: f32 fused multiply-add chains (the reference's SIMD builds do the same); a score that moves by an ulp can
    # move one fp16-rounded exp() by 2^-11, hence the looser bound. The exact order is pinned by the whole-model tests
    # against the oracle's restatement of it (orc_set_sum_order(2)).
    assert relrms(got, exp) <= 2e-3, relrms(got, exp)
    print("attention bit-identical elements (f64 order):", float((got64 == exp).mean()), " default vs f64:", relrms(got, got64))


def test_softmax_golden_through_attention(oracle, golden):
    """golden soft_max rows (scale + causal mask + fp16-table exp) reproduced by the attention kernel with V = I"""
    L = g.load()
    gb = golden["block_ops"]
    kq = gb["sm_kq"]                            # [n_head=4, N=3, n_kv=40] raw K.Q values
    n_past = int(gb["sm_n_past"])
    H, N, n_kv = kq.shape
    D = 64
    # choose q = e_0 * 1 and K[j] = kq value in component 0 so that K.Q reproduces kq for head h, token t: needs one
    # kv head per (h, t) pair -> run each (h, t) as its own single-head launch
    for h in range(H):
        for t in range(N):
            nk = n_past + t + 1
            q = np.zeros((1, 3, D), np.float32)
            q[0, 0, 0] = 1.0
            kc = np.zeros((nk, 1, D), np.float32)
            kc[:, 0, 0] = kq[h, t, :nk]
            vc = np.zeros((nk, 1, D), np.float32)
            vc[:min(nk, D), 0, :][np.arange(min(nk, D)), np.arange(min(nk, D))] = 1.0      # V = identity on the first 64 keys
            qb, kb, vb, o = g.DevBuf(host=q), g.DevBuf(host=kc), g.DevBuf(host=vc), g.DevBuf(D * 4)
            L.ggml_hip_attention(qb.ptr, 1, 1, 1, D, nk - 1, kb.ptr, vb.ptr, o.ptr)
            got = o.to_host(np.float32, (D,))
            assert np.array_equal(got[:min(nk, D)], gb["sm_p"][h, t, :min(nk, D)])


@pytest.mark.parametrize("H,HKV,N,n_past", [(4, 1, 32, 0), (8, 2, 45, 5), (3, 1, 100, 37), (2, 2, 33, 64), (5, 1, 700, 0), (2, 1, 17 * 16, 1500),
                                            (3, 1, 2048, 0), (16, 8, 513, 1790), (2, 1, 70, 2390)])
def test_prefill_attention_forms_are_bit_identical(H, HKV, N, n_past):
    """the prefill attention kernels on the f32 matrix pipe -- k_attention_mfma (32-token tiles, scores in the global scratch: pinned against the oracle's
    dot_qk_mfma / dot_pv_mfma by the whole-model tests; form 32), k_attention_flash (round 5, the default while 32 rows of fp16 probabilities fit LDS: K.Q run
    twice, nothing leaves the CU; forms 0 and 1 -- beyond ~2370 keys form 0 IS the scratch form), k_attention_mfma16 (16-token tiles, f32 scores in LDS) and
    k_attention_mfma16h (16-token tiles, K.Q twice, fp16 probabilities in LDS: two workgroups per CU) -- give the same bits: ragged last tiles, a context that
    does not start at 0, MQA and GQA, a full 2048-token prompt (ggml.c:10911-11102 soft_max, 12389-12456 the two dot products)"""
    L = g.load()
    D = 64
    rng = np.random.default_rng(H * 1000 + N + n_past)
    n_kv = n_past + N
    qkv = rng.standard_normal((N, H + 2 * HKV, D)).astype(np.float32)
    kc = rng.standard_normal((n_kv, HKV, D)).astype(np.float32)
    vc = rng.standard_normal((n_kv, HKV, D)).astype(np.float32)
    qb, kb, vb, ob_ = g.DevBuf(host=qkv), g.DevBuf(host=kc), g.DevBuf(host=vc), g.DevBuf(N * H * D * 4)
    outs = {}
    try:
        for form in (32, 0, 1, 16, 17):
            L.ggml_hip_debug_attention_form(form)
            L.ggml_hip_memset(ob_.ptr, 0xFF, N * H * D * 4)
            L.ggml_hip_attention(qb.ptr, N, H, HKV, D, n_past, kb.ptr, vb.ptr, ob_.ptr)
            outs[form] = ob_.to_host(np.float32, (N, H * D))
    finally:
        L.ggml_hip_debug_attention_form(0)
        for b in (qb, kb, vb, ob_):
            b.free()
    assert np.isfinite(outs[32]).all()
    for form in (0, 1, 16, 17):
        assert np.array_equal(outs[form], outs[32]), f"form {form}"


@pytest.mark.parametrize("H,HKV,N,n_past", [(4, 1, 512, 3584), (3, 1, 512, 7680), (4, 2, 512, 15872), (2, 1, 513, 5000), (8, 8, 33, 2400), (2, 1, 512, 2048), (2, 1, 96, 8000)])
def test_prefill_attention_long_contexts_keep_the_flash_form(H, HKV, N, n_past):
    """round 6: beyond 2368 keys (74 tiles) k_attention_flash runs its LONG form -- the LDS rows hold a chunk of 64 key tiles, K.Q is run for the row maxima, again
    for the row sums and a third time chunk by chunk in front of V.P, whose accumulators live across the chunks -- instead of handing the launch to the scratch
    form (k_attention_mfma: the N x n_kv score matrix through HBM four times). Same chains, same operands, same order: bit-identical to the scratch form (32) at
    4096 / 8192 / 16384 keys with 512-token batches (BASELINE config 5's batches; the reference's 8k-16k range, README.md:9; semantics ggml.c:12389-12456,
    libfalcon.cpp:2285-2366), ragged last tiles, a chunk boundary inside the batch's causal triangle, MQA and GQA"""
    L = g.load()
    D = 64
    rng = np.random.default_rng(H * 1000 + N + n_past)
    n_kv = n_past + N
    qkv = rng.standard_normal((N, H + 2 * HKV, D)).astype(np.float32)
    kc = rng.standard_normal((n_kv, HKV, D)).astype(np.float32)
    vc = rng.standard_normal((n_kv, HKV, D)).astype(np.float32)
    qb, kb, vb, ob_ = g.DevBuf(host=qkv), g.DevBuf(host=kc), g.DevBuf(host=vc), g.DevBuf(N * H * D * 4)
    outs = {}
    try:
        for form in (32, 0):
            L.ggml_hip_debug_attention_form(form)
            L.ggml_hip_memset(ob_.ptr, 0xFF, N * H * D * 4)
            L.ggml_hip_attention(qb.ptr, N, H, HKV, D, n_past, kb.ptr, vb.ptr, ob_.ptr)
            outs[form] = ob_.to_host(np.float32, (N, H * D))
        plan = (ctypes.c_longlong * 16)()
        L.ggml_hip_debug_attention_plan(N, H, HKV, D, n_past, plan)         # form 0 is still set: what it planned
    finally:
        L.ggml_hip_debug_attention_form(0)
        for b in (qb, kb, vb, ob_):
            b.free()
    assert (plan[0], plan[2], plan[3], plan[4]) == (FLASH, 64, 0, 1), list(plan)      # k_attention_flash, chunks of 64 key tiles, not KEEP, LONG (csrc/fq_attn_forms.h)
    assert np.isfinite(outs[32]).all()
    assert np.array_equal(outs[0], outs[32])


@pytest.mark.parametrize("env", [{"FQ_ATTN_KEEP": "0"}, {"FQ_ATTN_PERSIST": "0"}, {"FQ_ATTN_KEEP": "0", "FQ_ATTN_PERSIST": "0", "FQ_ATTN_PACK_MIN_N": "100000"}])
def test_flash_attention_switches_keep_the_bits(env):
    """the prefill attention's A/B switches -- K.Q run twice instead of a wave's score tiles kept in registers, one workgroup per item instead of persistent ones, keys
    not re-laid in operand order -- select other code, not other results: in a process of their own (the switches are read once) the flash form still equals the
    scratch form bit for bit at 1536 / 288 / 96 tokens of 71 heads (48 / 9 / 3 key tiles: all three pitch instantiations)"""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "gpu_attn_forms.py"), "1536", "288", "96"], env=dict(os.environ, FORMS="32,1", **env),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if "form  1" in l]
    assert len(lines) == 3 and all(l.rstrip().endswith("True") for l in lines), r.stdout


# ---- the launcher branches behind switches that are read once per process: a child process each, one at a time (scripts/gpu_attn_plan_case.py)
ONE_ROW, ROWS_LDS, ROWS_SCRATCH, FLASH, MFMA_SCRATCH = 2, 3, 4, 5, 8         # fq_attn_family, FQ_AF_* (csrc/fq_attn_forms.h)
SWITCH_CASES = [({"FQ_ATTN_ROWS": "8"}, 9, 100, (ROWS_LDS, 8)), ({"FQ_ATTN_ROWS": "4"}, 9, 100, (ROWS_LDS, 4)), ({"FQ_ATTN_ROWS": "2"}, 9, 100, (ROWS_LDS, 2)),
                ({"FQ_ATTN_ROWS": "0"}, 9, 100, (ONE_ROW, 1)), ({"FQ_ATTN_MFMA": "0"}, 40, 60, (ROWS_LDS, 4)), ({"FQ_ATTN_SCRATCH": "0"}, 6, 3500, (ROWS_LDS, 2)),
                ({"FQ_ATTN_FLASH": "0"}, 33, 5, (MFMA_SCRATCH, 32)), ({"FQ_ATTN_FLASH_LONG": "0"}, 33, 2400, (MFMA_SCRATCH, 32))]
_switch_refs = {}


@pytest.mark.parametrize("env,N,n_past,want", SWITCH_CASES, ids=["-".join(f"{k[8:]}={v}" for k, v in c[0].items()) for c in SWITCH_CASES])
def test_attention_switches_reach_their_plans(oracle, tmp_path, env, N, n_past, want):
    """FQ_ATTN_ROWS / _MFMA / _SCRATCH / _FLASH / _FLASH_LONG select other kernels of the prompt attention, not other results: the child reports the plan the
    launcher took (family, tokens per workgroup) and its outputs -- the rows forms within test_attention's bounds of the plain f64 attention (2e-6 in reference
    order, 2e-3 in the default order: f32 multiply-add chains and one fp16-rounded exp() per ulp of a score), the matrix-pipe forms bit for bit form 32's"""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "scripts"))
    try:
        from gpu_attn_plan_case import attn_case_inputs
    finally:
        sys.path.pop(0)
    H, HKV = 2, 1
    out = str(tmp_path / "case.npz")
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "gpu_attn_plan_case.py"), str(H), str(HKV), str(N), str(n_past), out],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    res = np.load(out)
    assert (int(res["plan"][0]), int(res["plan"][1])) == want, r.stdout
    assert f"plan family {want[0]} R {want[1]} " in r.stdout, r.stdout
    if want[0] == MFMA_SCRATCH:
        assert np.isfinite(res["got32"]).all() and np.array_equal(res["got"], res["got32"])
    else:
        if (N, n_past) not in _switch_refs:
            qkv, kc, vc = attn_case_inputs(H, HKV, N, n_past)
            _switch_refs[(N, n_past)] = _attention_ref(oracle, qkv[:, :H], kc, vc, n_past, H, HKV)
        exp = _switch_refs[(N, n_past)]
        print("rel. error, reference order:", relrms(res["got64"], exp), " default order:", relrms(res["got"], exp))
        assert relrms(res["got64"], exp) <= 2e-6, relrms(res["got64"], exp)
        assert relrms(res["got"], exp) <= 2e-3, relrms(res["got"], exp)
