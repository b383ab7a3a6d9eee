"""GPU: the operator ABI of include/ggml-hip-ops.h beyond the sums -- epilogues, strides and write extents, per form.

Every output lives in a guard (tests/guard.py): a front guard, the gaps between rows that `ldd > M` leaves, and a back guard that
covers the tile the kernels round the matrix up to, all holding one NaN bit pattern that must still be there after the launch; the
gaps of the inputs hold 1e30. Expected values come from the oracle (oracle/), never from the device, and are compared bit for bit
unless a test says otherwise. Which form ran is asserted by the cases of section 2b only; elsewhere the shapes are the smallest that land in each form by the launchers'
own rules (csrc/ggml_hip_ops.hip fq_mul_mat_q_acts, csrc/kernels_gemm.hip fq_launch_gemm, csrc/kernels_gemm_skinny.hip
fq_launch_gemm_skinny, csrc/kernels_gemm_skinny_k.hip fq_skinny_q4k_shape), named in the comment next to each."""
import ctypes as C

import numpy as np
import pytest

import ggllm_cpp_amd as g
import guard
import mm_keys
import mm_shapes as ms
import synth
from decode_attn import attention_ref
import decode_attn as da
from oracle import binding as ob

pytestmark = pytest.mark.gpu

STORE, GELU, ADD2, ADD2_INPLACE = 0, 1, 2, 3
EPI_NAME = {STORE: "STORE", GELU: "GELU", ADD2: "ADD2", ADD2_INPLACE: "ADD2 in place"}
LDD_PAD = 67            # odd and wider than a 64-row tile tail: every tail row of every column lands in a gap
LDX_PAD = 36            # a multiple of 4 (the quantizers load float4), not of 32
COL_SCALE = np.array([1e-3, 0.05, 1.0, 30.0], np.float32)      # column n of x: the GELU lookup sees fp16 subnormals through values of tens


@pytest.fixture(scope="module", autouse=True)
def _init():
    g.init(0)


# ------------------------------------------------------------------------------------------------ orders
# mode -> (switch, the orc_set_sum_order that restates it for N columns), as tests/test_gpu_mul_mat.py pins the sums
def _oracle_order(mode, N):
    if mode == "default":
        return 2                                   # the backend's own choice per shape (wave order for N <= 4, K-split partial sums above)
    if mode == "seq":
        return 5 if N > g_max_gemv_cols() else 2   # ggml_hip_gemm_sequential is the prefill GEMM's switch (N > 4); the mat-vec kernels keep their order
    if mode in ("ref1", "ref2"):
        return 0                                   # the reference's scalar build
    return {"cfg0": 5, "cfg1": 3, "cfg3": 4, "cfg6": 4, "cfg7": 3}[mode]      # FQ_GEMM_CFG: <1,4> S = 1; <4,1> / <4,4,2> S = 4; <2,4> / <2,4,2> S = 2 (the backend's table: fq_mm_cfg_split, csrc/fq_mm_forms.h; restated here on purpose)


def g_max_gemv_cols():
    return 4                                       # FQ_GEMV_MAX_COLS (csrc/kernels.h)


class _mode:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        L = g.load()
        if self.mode == "seq":
            L.ggml_hip_gemm_sequential(1)
        elif self.mode == "ref1":
            L.ggml_hip_reference_order(1)
        elif self.mode == "ref2":
            L.ggml_hip_reference_order(2)

    def __exit__(self, *a):
        L = g.load()
        if self.mode == "seq":
            L.ggml_hip_gemm_sequential(0)
        elif self.mode in ("ref1", "ref2"):
            L.ggml_hip_reference_order(0)


def _oracle_mul_mat(oracle, order, t, w, K, M, x):
    oracle.lib.orc_set_sum_order(order)
    try:
        return oracle.mul_mat(t, w, K, M, x, 8)
    finally:
        oracle.lib.orc_set_sum_order(0)


def _diff(got, exp):
    d = np.flatnonzero(got.view(np.uint32).ravel() != exp.view(np.uint32).ravel())
    if not d.size:
        return ""
    n, m = divmod(int(d[0]), got.shape[1])
    unwritten = int((got.view(np.uint32).ravel()[d] == guard.NAN_BITS).sum())
    return (f"{d.size} of {got.size} values differ ({unwritten} never written), first at column {n} row {m}: "
            f"{got[n, m]!r} != {exp[n, m]!r}")


def _inputs(oracle, t, K, M, N, seed):
    rng = np.random.default_rng(seed)
    # (tall matrices: random valid blocks drawn in quantized space, not hundreds of millions of floats through the quantizer)
    w = synth.random_blocks(t, M, K, rng) if M > 1024 else synth.quantized_matrix(oracle, t, M, K, rng)
    x = rng.standard_normal((N, K)).astype(np.float32) * COL_SCALE[np.arange(N) % 4][:, None]
    a1 = rng.standard_normal((N, M)).astype(np.float32)
    a2 = rng.standard_normal((N, M)).astype(np.float32)
    return w, x, a1, a2


def _device_key(dw, t, N):
    out = (C.c_longlong * mm_keys.KEY_LEN)()
    g.load().ggml_hip_debug_mul_mat_plan(dw.h, N, out)
    return (t,) + tuple(int(v) for v in out)


def _mat_mul_case(oracle, t, K, M, N, mode="default", epilogues=(STORE, GELU, ADD2, ADD2_INPLACE), ldx_launch=True, check_key=False):
    """one weight matrix, one set of columns: every epilogue at ldd = M and ldd = M + 67 into guarded outputs through
    ggml_hip_mul_mat_q_acts, then ggml_hip_mul_mat_q with ldx = K + 36; returns the list of complaints. check_key: the launch this device plans for the shape
    (ggml_hip_debug_mul_mat_plan) must be the one the CPU census (tests/test_mm_coverage_cpu.py) counted the shape for, at 256 CUs"""
    L = g.load()
    w, x, a1, a2 = _inputs(oracle, t, K, M, N, seed=(K * 131 + M) * 131 + N * 17 + t)
    base = _oracle_mul_mat(oracle, _oracle_order(mode, N), t, w, K, M, x)
    assert np.isfinite(base).all()
    exp = {STORE: base, ADD2: (base + a1) + a2}
    exp[ADD2_INPLACE] = exp[ADD2]
    if GELU in epilogues:
        exp[GELU] = oracle.gelu(base)
        assert np.isfinite(exp[GELU]).all()
    bad = []
    dw = g.Weight(t, w, K, M)
    acts = L.ggml_hip_acts_alloc(ob.VEC_DOT[t], K, N)
    xg = guard.in_guard(x)
    bufs = [xg]
    try:
        with _mode(mode):
            if check_key:
                want, have = mm_keys.key(t, K, M, N, mode), _device_key(dw, t, N)
                assert have == want, f"{ob.TYPE_NAME[t]} K {K} M {M} N {N} [{mode}]: this device plans launch key {have}, the census counted the shape as {want}"
            L.ggml_hip_quantize_acts(acts, xg.ptr, K, N)
            for ldd in (M, M + LDD_PAD):
                b1, b2 = guard.in_guard(a1, ldd), guard.in_guard(a2, ldd)
                bufs += [b1, b2]
                for epi in epilogues:
                    out = guard.out_guard(N, M, ldd, payload=a2 if epi == ADD2_INPLACE else None)
                    bufs.append(out)
                    if epi in (STORE, GELU):
                        L.ggml_hip_mul_mat_q_acts(dw.h, acts, N, out.ptr, ldd, epi, None, None)
                    else:
                        L.ggml_hip_mul_mat_q_acts(dw.h, acts, N, out.ptr, ldd, ADD2, b1.ptr, out.ptr if epi == ADD2_INPLACE else b2.ptr)
                    L.ggml_hip_synchronize()
                    where = f"{EPI_NAME[epi]}, ldd = {ldd}"
                    try:
                        got = out.check()
                    except guard.GuardError as e:
                        bad.append(f"{where}: {e}")
                        continue
                    if not np.array_equal(got, exp[epi]):
                        bad.append(f"{where}: {_diff(got, exp[epi])}")
                for name, b in (("add1", b1), ("add2", b2)):
                    try:
                        b.check()
                    except guard.GuardError as e:
                        bad.append(f"{name} at stride {ldd} was written: {e}")
            if ldx_launch:
                ldx, ldd = K + LDX_PAD, M + LDD_PAD
                xs, out = guard.in_guard(x, ldx), guard.out_guard(N, M, ldd)
                bufs += [xs, out]
                L.ggml_hip_mul_mat_q(dw.h, xs.ptr, ldx, N, out.ptr, ldd)
                try:
                    got = out.check()
                    if not np.array_equal(got, base):
                        bad.append(f"ggml_hip_mul_mat_q, ldx = {ldx}: {_diff(got, base)}")
                    xs.check()
                except guard.GuardError as e:
                    bad.append(f"ggml_hip_mul_mat_q, ldx = {ldx}: {e}")
    finally:
        for b in bufs:
            b.free()
        L.ggml_hip_acts_free(acts)
        dw.free()
    return [f"{ob.TYPE_NAME[t]} K {K} M {M} N {N} [{mode}]: {b}" for b in bad]


def _assert_none(bad):
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ 2. mat-mul, per form
@pytest.mark.parametrize("N", ms.MAT_VEC[2])
@pytest.mark.parametrize("t", ob.WEIGHT_TYPES)
def test_mat_vec_columns(oracle, t, N):
    """k_gemv<NCOLS>: 1 column, 2, 2 + 1 (two launches: the second at add1 + 2 * ld_add) and 4"""
    K, M, _ = ms.MAT_VEC
    _assert_none(_mat_mul_case(oracle, t, K, M, N))


LEGACY_FORMS = ms.LEGACY_FORMS        # (the shapes and the form each lands in: tests/mm_shapes.py)


@pytest.mark.parametrize("K,M,N", LEGACY_FORMS)
@pytest.mark.parametrize("t", ob.LEGACY)
def test_legacy_forms(oracle, t, K, M, N):
    _assert_none(_mat_mul_case(oracle, t, K, M, N))


@pytest.mark.parametrize("cfg", ms.LEGACY_TILE_CFGS)
@pytest.mark.parametrize("t", ob.LEGACY)
def test_legacy_tile_instantiations(oracle, t, cfg, monkeypatch):
    """FQ_GEMM_CFG (read per call): k_gemm_q<4, 1> (32-token tiles: two tile rows of tokens), <2, 4>, <2, 4, 2> and <4, 4, 2> (64-row workgroups: 70 rows = a
    whole and a 6-row workgroup), 40 columns of a 128-token tile"""
    monkeypatch.setenv("FQ_GEMM_CFG", str(cfg))
    _assert_none(_mat_mul_case(oracle, t, *ms.TILE_INSTANTIATION, mode=f"cfg{cfg}"))


@pytest.mark.parametrize("t", ob.LEGACY)
def test_legacy_single_sum_tile(oracle, t, monkeypatch):
    """FQ_GEMM_CFG=0: k_gemm_q<1, 4>, one left-to-right sum per row, at 130 columns (beyond SEQ16's 128: two token tile rows, the second of two columns)"""
    monkeypatch.setenv("FQ_GEMM_CFG", "0")
    _assert_none(_mat_mul_case(oracle, t, *ms.SINGLE_SUM_TILE, mode="cfg0"))


@pytest.mark.parametrize("t", ob.LEGACY)
def test_legacy_seq16(oracle, t):
    """ggml_hip_gemm_sequential(1), 17..128 columns of a legacy format: k_gemm_q<4, 4, 1, SEQ16>, sixteen 16 x 16 tiles per workgroup"""
    _assert_none(_mat_mul_case(oracle, t, *ms.SEQ16, mode="seq"))


KQUANT_FORMS = ms.KQUANT_FORMS


@pytest.mark.parametrize("K,M,N", KQUANT_FORMS)
@pytest.mark.parametrize("t", ob.KQUANTS)
def test_kquant_forms(oracle, t, K, M, N):
    _assert_none(_mat_mul_case(oracle, t, K, M, N))


@pytest.mark.parametrize("cfg", ms.KQUANT_TILE_CFGS)
@pytest.mark.parametrize("t", ob.KQUANTS)
def test_kquant_tile_instantiations(oracle, t, cfg, monkeypatch):
    """FQ_GEMM_CFG: k_gemm_q<4, 1>, <2, 4> and <2, 4, 2> of the k-quants (<4, 4, 2> is not theirs: register budget)"""
    monkeypatch.setenv("FQ_GEMM_CFG", str(cfg))
    _assert_none(_mat_mul_case(oracle, t, *ms.TILE_INSTANTIATION, mode=f"cfg{cfg}"))


# one mat-vec, one small-batch and one tile shape per family under the three other orders:
#   seq   ggml_hip_gemm_sequential(1): N > 4 through S = 1 (legacy 5..16 columns: the resident form with one K share; k-quants: k_gemm_q<1, 4>)
#   ref1  ggml_hip_reference_order(1): k_mul_mat_ref, one thread per output
#   ref2  ggml_hip_reference_order(2): legacy N = 1 k_gemv_legacy_ref, N >= 2 the GEMM with S = 1; k-quants k_gemv_kq_ref column by column
ORDER_SHAPES = ms.ORDER_SHAPES


@pytest.mark.parametrize("mode", ms.ORDER_MODES)
@pytest.mark.parametrize("t", ob.WEIGHT_TYPES)
def test_orders(oracle, t, mode):
    bad = []
    for K, M, N in ORDER_SHAPES["legacy" if t in ob.LEGACY else "kquant"]:
        bad += _mat_mul_case(oracle, t, K, M, N, mode=mode)
    if t in ob.LEGACY and mode == "ref2":
        bad += _mat_mul_case(oracle, t, 512, 37, 1, mode=mode)      # k_gemv_legacy_ref (N = 3 above already runs the GEMM)
    _assert_none(bad)


# ------------------------------------------------------------------------------------------------ 2b. the forms only model-sized matrices reach
# tests/test_mm_coverage_cpu.py holds the launch keys of these shapes (and of every list above) against those of the Falcon-7B / 40B / 180B matrices; each case
# asserts that this device plans the key the census counted it for.
def _case_id(c):
    t, K, M, N, mode = c
    return f"{ob.TYPE_NAME[t]}-{K}-{M}-{N}-{mode}"


@pytest.mark.parametrize("case", ms.model_forms_legacy_cases(), ids=_case_id)
def test_legacy_model_forms(oracle, case):
    """k_gemm_skinny_res / k_gemm_skinny at two K shares (more than 32 736 rows), persistent workgroups that loop over row pairs (more than 8192 rows), the
    K-share form at 2, 5 and 8 tiles per workgroup, with and without the row-block walk: every epilogue, ldd = M and M + 67, ldx = K + 36, guarded, bit for bit"""
    t, K, M, N, mode = case
    _assert_none(_mat_mul_case(oracle, t, K, M, N, mode=mode, check_key=True))


@pytest.mark.parametrize("case", ms.model_forms_further_cases(), ids=_case_id)
def test_model_forms_further(oracle, case):
    """the keys the census named beyond the legacy table: second passes per weight-stage count, the k-quants' streaming forms at two K shares"""
    t, K, M, N, mode = case
    _assert_none(_mat_mul_case(oracle, t, K, M, N, mode=mode, check_key=True))


@pytest.mark.parametrize("mode", sorted(ms.TILE_FORMS_EVEN))
@pytest.mark.parametrize("t", ob.WEIGHT_TYPES)
def test_tile_forms_even(oracle, t, mode, monkeypatch):
    """the tile GEMM on whole 64-row workgroups (every model matrix is a multiple of 64 rows; the shapes above end in ragged tiles): one token tile, a whole one
    and a second ragged one per cfg"""
    if mode.startswith("cfg"):
        monkeypatch.setenv("FQ_GEMM_CFG", mode[3:])
    K, M = ms.TILE_FORMS_EVEN_KM
    bad = []
    for N in ms.TILE_FORMS_EVEN[mode]:
        bad += _mat_mul_case(oracle, t, K, M, N, mode=mode, check_key=True)
    _assert_none(bad)


# ------------------------------------------------------------------------------------------------ 3. few blocks, few rows
# The K loops, read for 1 to 5 stages / blocks before these ran on a device:
#   k_gemv             units beyond the row are clamped to its last unit and masked (fq_unit_load_col); one unit (K = 32) is one live lane
#   k_gemm_q           a stage is 4 blocks; g0_of() re-reads the last stage beyond the end, groups beyond K are committed as zeros, the token scales of a short
#                      row (fewer than 4 blocks) are read from block 0 and masked by `g0 + gg < ngroups`; the pair form issues stages 0..3 up front through the same clamp
#   k_gemm_skinny*     a stage is 32 blocks, so these rows are one partial stage; the prologues are bounded by `s < nstages`, the DMA sources by the image's last
#                      16 bytes and by rows re-read inside the weight slab's slack
#   k-quants           2 super-blocks at most here: the mat-vec kernels and the tile GEMM (the small-batch forms start at 8 super-blocks, fq_skinny_q4k_shape)
FEW_M, FEW_N = ms.FEW_M, ms.FEW_N


def _few_blocks(oracle, t, K):
    bad = []
    for M in FEW_M:
        for N in FEW_N:
            for mode in ("default", "seq"):
                bad += _mat_mul_case(oracle, t, K, M, N, mode=mode, epilogues=(STORE, ADD2), ldx_launch=False)
    return bad


@pytest.mark.parametrize("K", ms.FEW_K_LEGACY)
@pytest.mark.parametrize("t", ob.LEGACY)
def test_few_blocks_legacy(oracle, t, K):
    _assert_none(_few_blocks(oracle, t, K))


@pytest.mark.parametrize("K", ms.FEW_K_KQUANTS)
@pytest.mark.parametrize("t", ob.KQUANTS)
def test_few_blocks_kquants(oracle, t, K):
    _assert_none(_few_blocks(oracle, t, K))


# ------------------------------------------------------------------------------------------------ 4. the other operators
def relrms(a, b):
    return float(np.abs(a.astype(np.float64) - b).max() / (np.sqrt((b.astype(np.float64) ** 2).mean()) + 1e-30))


def _attention_inputs(H, HKV, N, n_past):
    rng = np.random.default_rng(H * 1000 + N + n_past)
    n_kv = n_past + N
    qkv = rng.standard_normal((N, H + 2 * HKV, 64)).astype(np.float32)
    kc = rng.standard_normal((n_kv, HKV, 64)).astype(np.float32)
    vc = rng.standard_normal((n_kv, HKV, 64)).astype(np.float32)
    return qkv, kc, vc


def _attention_guarded(qb, kb, vb, N, H, HKV, n_past):
    L = g.load()
    out = guard.out_guard(N, H * 64)
    try:
        L.ggml_hip_attention(qb.ptr, N, H, HKV, 64, n_past, kb.ptr, vb.ptr, out.ptr)
        L.ggml_hip_synchronize()
        return out.check()
    finally:
        out.free()


# (33 tokens: one whole 32-token tile and a tile of one token; 45: a ragged 16-token tile as well, GQA, a context that starts at 0; 70 tokens behind 2390
#  keys: beyond the 74 key tiles whose probabilities fit LDS -- form 0 is then the flash kernel's long form)
@pytest.mark.parametrize("H,HKV,N,n_past", [(3, 1, 33, 5), (8, 2, 45, 0), (2, 1, 70, 2390)])
def test_prefill_attention_forms_guarded(oracle, H, HKV, N, n_past):
    """every prefill attention form writes att[N][H * 64] and nothing else -- the ragged last token tile's rows beyond N stay in the guard -- and gives form 32's
    bits; form 32 against the plain numpy f64 attention at test_attention's own bounds"""
    L = g.load()
    qkv, kc, vc = _attention_inputs(H, HKV, N, n_past)
    qb, kb, vb = g.DevBuf(host=qkv), g.DevBuf(host=kc), g.DevBuf(host=vc)
    outs, bad = {}, []
    try:
        for form in (32, 0, 1, 16, 17):
            L.ggml_hip_debug_attention_form(form)
            try:
                outs[form] = _attention_guarded(qb, kb, vb, N, H, HKV, n_past)
            except guard.GuardError as e:
                bad.append(f"form {form}: {e}")
        L.ggml_hip_debug_attention_form(32)
        L.ggml_hip_reference_order(1)
        try:
            got64 = _attention_guarded(qb, kb, vb, N, H, HKV, n_past)
        except guard.GuardError as e:
            bad.append(f"form 32, f64: {e}")
            got64 = None
    finally:
        L.ggml_hip_reference_order(0)
        L.ggml_hip_debug_attention_form(0)
        for b in (qb, kb, vb):
            b.free()
    _assert_none(bad)
    for form in (0, 1, 16, 17):
        assert np.array_equal(outs[form], outs[32]), f"form {form}"
    exp = attention_ref(oracle, qkv[:, :H], kc, vc, n_past, H, HKV)
    assert relrms(got64, exp) <= 2e-6, relrms(got64, exp)
    assert relrms(outs[32], exp) <= 2e-3, relrms(outs[32], exp)


@pytest.mark.parametrize("H,HKV,N,n_past", [(3, 1, 7, 0), (2, 1, 16, 3500)])
def test_short_attention_routes_guarded(oracle, H, HKV, N, n_past):
    """fewer than 32 tokens: k_attention (one workgroup per head and token) and, beyond 3000 keys, k_attention_rows"""
    L = g.load()
    qkv, kc, vc = _attention_inputs(H, HKV, N, n_past)
    qb, kb, vb = g.DevBuf(host=qkv), g.DevBuf(host=kc), g.DevBuf(host=vc)
    try:
        got = _attention_guarded(qb, kb, vb, N, H, HKV, n_past)
        L.ggml_hip_reference_order(1)
        got64 = _attention_guarded(qb, kb, vb, N, H, HKV, n_past)
    finally:
        L.ggml_hip_reference_order(0)
        for b in (qb, kb, vb):
            b.free()
    exp = attention_ref(oracle, qkv[:, :H], kc, vc, n_past, H, HKV)
    assert relrms(got64, exp) <= 2e-6, relrms(got64, exp)
    assert relrms(got, exp) <= 2e-3, relrms(got, exp)


@pytest.mark.parametrize("pos_stride", [0, 1])
@pytest.mark.parametrize("n_seq", [1, 5])
def test_attention_decode_rows_guarded(oracle, n_seq, pos_stride):
    """ggml_hip_attention_decode (k_attn_decode for one row at pos_dev[0], k_attn_decode_seqs otherwise) writes att[n_seq][H * 64] and nothing around it; the
    rows equal the oracle's orc_attention_decode in the backend's order, bit for bit"""
    L = g.load()
    H, HKV, max_n_kv = 8, 2, 300
    positions = [257, 0, 129, 299, 16][:n_seq] if pos_stride else [257] * n_seq
    cases = [da.random_case(oracle, H, HKV, p, da.case_seed(H, HKV, p, salt=50 + s)) for s, p in enumerate(positions)]
    rng = np.random.default_rng(n_seq)
    caches = [da.build_cache(c, max_n_kv, da.FILL_RANDOM, rng) for c in cases]
    tab = L.ggml_hip_rope_table_create(da.D, max_n_kv, da.ROPE_CTX)
    qb = g.DevBuf(host=np.stack([c.qkv for c in cases]))
    kb, vb = g.DevBuf(host=np.stack([k for k, _ in caches])), g.DevBuf(host=np.stack([v for _, v in caches]))
    pb = g.DevBuf(host=np.array(positions, np.int32))
    out = guard.out_guard(n_seq, H * 64)
    try:
        L.ggml_hip_attention_decode(qb.ptr, n_seq, H, HKV, pb.ptr, pos_stride, max_n_kv, tab, kb.ptr, vb.ptr, max_n_kv * HKV * da.D, out.ptr, None, 0)
        L.ggml_hip_synchronize()
        att = out.check()
    finally:
        for b in (qb, kb, vb, pb, out):
            b.free()
        L.ggml_hip_free(tab)
    for s, c in enumerate(cases):
        assert np.array_equal(att[s], c.expected(oracle, 2)), f"sequence {s} at position {c.n_past}"


@pytest.mark.parametrize("N", [1, 3, 33])
@pytest.mark.parametrize("n_past", [0, 1021])
@pytest.mark.parametrize("H,HKV", [(8, 2), (16, 8)])
def test_rope_kv_store_guarded(oracle, H, HKV, n_past, N):
    """Q rotated in place and K rotated into the cache equal oracle.rope bit for bit, V is copied, the K / V slots of qkv and every cache row outside
    [n_past, n_past + N) -- five rows behind the batch included -- keep their bits"""
    L = g.load()
    D, n_ctx = 64, 2048
    rng = np.random.default_rng(H * 100 + n_past + N)
    qkv = rng.standard_normal((N, H + 2 * HKV, D)).astype(np.float32)
    rows = n_past + N + 5
    tab = L.ggml_hip_rope_table_create(D, n_past + N, n_ctx)
    qg = guard.Guard(N, (H + 2 * HKV) * D, payload=qkv).to_device()
    kg, vg = guard.out_guard(rows, HKV * D), guard.out_guard(rows, HKV * D)
    try:
        L.ggml_hip_rope_kv_store(qg.ptr, N, H, HKV, D, n_past, tab, kg.ptr, vg.ptr)
        L.ggml_hip_synchronize()
        out = qg.check().reshape(N, H + 2 * HKV, D)
        kc, vc = kg.check().reshape(rows, HKV, D), vg.check().reshape(rows, HKV, D)
    finally:
        for b in (qg, kg, vg):
            b.free()
        L.ggml_hip_free(tab)
    ref = oracle.rope(qkv[:, :H + HKV], D, H + HKV, N, n_past, n_ctx)
    assert np.array_equal(out[:, :H], ref[:, :H])
    assert np.array_equal(kc[n_past:n_past + N], ref[:, H:])
    assert np.array_equal(vc[n_past:n_past + N], qkv[:, H + HKV:])
    assert np.array_equal(out[:, H:], qkv[:, H:])
    live = np.zeros(rows, bool)
    live[n_past:n_past + N] = True
    for name, c in (("key", kc), ("value", vc)):
        assert (c[~live].view(np.uint32) == guard.NAN_BITS).all(), f"{name} cache rows outside [{n_past}, {n_past + N}) were written"


ACT_K = [(ob.Q8_0, 32), (ob.Q8_0, 64), (ob.Q8_0, 96), (ob.Q8_1, 32), (ob.Q8_1, 64), (ob.Q8_1, 96), (ob.Q8_K, 256), (ob.Q8_K, 512)]


def _act_rows(oracle, at, x):
    return np.stack([oracle.quantize_act(at, r) for r in x])


def _export(acts, at, K, n):
    L = g.load()
    nbytes = n * (K // ob.BLCK[at]) * ob.TSIZE[at]
    eb = g.DevBuf(nbytes)
    L.ggml_hip_acts_export(acts, n, eb.ptr)
    out = eb.to_host(np.uint8, (n, nbytes // n))
    eb.free()
    return out


@pytest.mark.parametrize("at,K", ACT_K)
def test_quantize_acts_strided(oracle, at, K):
    """ggml_hip_quantize_acts with ldx = K + 36 and 1e30 between the rows (k_quantize_q8's padded loop re-reads the last quad for its dead lanes; a stray
    1e30 would be the block's amax), one to five blocks per row: the exported blocks equal oracle.quantize_act bit for bit"""
    L = g.load()
    N = 5
    rng = np.random.default_rng(K + at)
    x = rng.standard_normal((N, K)).astype(np.float32) * COL_SCALE[np.arange(N) % 4][:, None]
    xg = guard.in_guard(x, K + LDX_PAD)
    acts = L.ggml_hip_acts_alloc(at, K, N)
    try:
        L.ggml_hip_quantize_acts(acts, xg.ptr, K + LDX_PAD, N)
        got = _export(acts, at, K, N)
        xg.check()
    finally:
        L.ggml_hip_acts_free(acts)
        xg.free()
    assert np.array_equal(got, _act_rows(oracle, at, x))


@pytest.mark.parametrize("at,K", [(ob.Q8_0, 96), (ob.Q8_1, 96), (ob.Q8_K, 512)])
def test_quantize_acts_leaves_the_other_columns(oracle, at, K):
    """four columns of A, then 1..3 columns of B into the same set: the columns beyond ncols still hold A (the quantizers' dead lanes store nothing)"""
    L = g.load()
    rng = np.random.default_rng(K * 3 + at)
    A = rng.standard_normal((4, K)).astype(np.float32)
    B = rng.standard_normal((4, K)).astype(np.float32) * 7
    eA, eB = _act_rows(oracle, at, A), _act_rows(oracle, at, B)
    ab, bb = g.DevBuf(host=A), g.DevBuf(host=B)
    acts = L.ggml_hip_acts_alloc(at, K, 4)
    try:
        for n in (1, 2, 3):
            L.ggml_hip_quantize_acts(acts, ab.ptr, K, 4)
            L.ggml_hip_quantize_acts(acts, bb.ptr, K, n)
            got = _export(acts, at, K, 4)
            assert np.array_equal(got[:n], eB[:n]), n
            assert np.array_equal(got[n:], eA[n:]), n
    finally:
        L.ggml_hip_acts_free(acts)
        ab.free()
        bb.free()


@pytest.mark.parametrize("t", ob.WEIGHT_TYPES)
def test_dequantize_rows_guarded(oracle, t):
    """repeated and out-of-order row lists, and the identity (rows_dev == NULL), into a guarded dst[nrows][K]"""
    L = g.load()
    K, M = 512, 37
    rng = np.random.default_rng(t)
    w = synth.quantized_matrix(oracle, t, M, K, rng)
    deq = np.stack([oracle.dequantize(t, w[r], K) for r in range(M)])
    dw = g.Weight(t, w, K, M)
    try:
        for rows in ([5, 5, 0, 36, 2, 36, 1], [36], None):
            n = M if rows is None else len(rows)
            rb = g.DevBuf(host=np.asarray(rows, np.int32)) if rows is not None else None
            out = guard.out_guard(n, K)
            try:
                L.ggml_hip_dequantize_rows(dw.h, rb.ptr if rb else None, n, out.ptr)
                L.ggml_hip_synchronize()
                got = out.check()
            finally:
                out.free()
                if rb:
                    rb.free()
            assert np.array_equal(got, deq if rows is None else deq[rows]), rows
    finally:
        dw.free()


# one length just past each grid cap: the first elements of the grid-stride loops' second trip
ELEMENTWISE_N = [1, 255, 257, 4096 * 256 + 3]
PATTERN = 4099           # a prime number of distinct inputs, tiled: the oracle's GELU is evaluated once per input


def _vector_out(n):
    return guard.out_guard(n, 1)       # n rows of one word: the back guard is 128 words plus the round-up to 128 rows


@pytest.mark.parametrize("n", ELEMENTWISE_N)
def test_gelu_guarded(oracle, n):
    L = g.load()
    rng = np.random.default_rng(n)
    pat = rng.standard_normal(PATTERN).astype(np.float32) * COL_SCALE[np.arange(PATTERN) % 4]
    pat[:6] = [0.0, -0.0, 6.0e-8, -3.0e-5, 11.0, -11.0]
    x = np.resize(pat, n)
    exp = np.resize(oracle.gelu(pat), n)
    xb, out = guard.in_guard(x.reshape(n, 1)), _vector_out(n)
    try:
        L.ggml_hip_gelu(xb.ptr, out.ptr, n)
        L.ggml_hip_synchronize()
        got = out.check().ravel()
    finally:
        xb.free()
        out.free()
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))


@pytest.mark.parametrize("n", ELEMENTWISE_N)
def test_add3_guarded(n):
    L = g.load()
    rng = np.random.default_rng(n + 1)
    a, b, c = (rng.standard_normal(n).astype(np.float32) * s for s in (np.float32(1.0), np.float32(1e-3), np.float32(100.0)))
    bufs = [guard.in_guard(v.reshape(n, 1)) for v in (a, b, c)]
    out = _vector_out(n)
    try:
        L.ggml_hip_add3(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, out.ptr, n)
        L.ggml_hip_synchronize()
        got = out.check().ravel()
    finally:
        for v in bufs + [out]:
            v.free()
    assert np.array_equal(got, (a + b) + c)


@pytest.mark.parametrize("n", [1, 255, 257, 8192 * 256 + 5])
def test_fp16_to_fp32_row_guarded(n):
    """all 65536 fp16 patterns, tiled (the short lengths: a window over the subnormal / normal boundary, another over infinities and NaNs): numpy's exact
    widening, bits for the non-NaN patterns, NaN for NaN"""
    L = g.load()
    every = np.arange(1 << 16, dtype=np.uint16)
    for start in ((0,) if n > 65536 else (0x03F0, 0x7BF0, 0xFBF0)):
        src = np.resize(np.roll(every, -start), n)
        exp = src.view(np.float16).astype(np.float32)
        sb, out = g.DevBuf(host=src), _vector_out(n)
        try:
            L.ggml_hip_fp16_to_fp32_row(sb.ptr, out.ptr, n)
            L.ggml_hip_synchronize()
            got = out.check().ravel()
        finally:
            sb.free()
            out.free()
        nan = np.isnan(exp)
        assert np.array_equal(got.view(np.uint32)[~nan], exp.view(np.uint32)[~nan])
        assert np.isnan(got[nan]).all()


@pytest.mark.parametrize("n", [64, 4544, 14848, 18176])
def test_layer_norm_guarded(oracle, n):
    """rows up to n_ff long (14848 and 18176 floats: more than the 64 KiB of dynamic LDS a kernel has by default, which the launcher grants), y guarded, the
    plain norm and * w + b against the oracle at test_layer_norm's own bound"""
    L = g.load()
    rows = 3
    rng = np.random.default_rng(n)
    x = (rng.standard_normal((rows, n)) * 3 + 0.5).astype(np.float32)
    w = (1 + 0.02 * rng.standard_normal(n)).astype(np.float32)
    b = (0.02 * rng.standard_normal(n)).astype(np.float32)
    xb, wb, bb = guard.in_guard(x), guard.in_guard(w[None]), guard.in_guard(b[None])
    got = {}
    try:
        for name, args in (("plain", (None, None)), ("full", (wb.ptr, bb.ptr))):
            out = guard.out_guard(rows, n)
            try:
                L.ggml_hip_layer_norm(xb.ptr, n, rows, args[0], args[1], out.ptr)
                L.ggml_hip_synchronize()
                got[name] = out.check()
            finally:
                out.free()
    finally:
        for v in (xb, wb, bb):
            v.free()
    for name, exp in (("plain", oracle.norm(x)), ("full", oracle.layer_norm(x, w, b))):
        assert not (got[name].view(np.uint32) == guard.NAN_BITS).any(), f"{name}: elements of y were never written"
        assert relrms(got[name], exp) <= 1e-6, (name, relrms(got[name], exp))


@pytest.mark.parametrize("n", [66, 40948])
def test_layer_norm_refuses_what_it_cannot_do(n, capfd):
    """a row that is no whole number of float4 vectors, or longer than the 160 KiB of LDS hold (40944 floats): a message, nothing launched, y untouched"""
    L = g.load()
    x = np.ones((2, n), np.float32)
    xb, out = g.DevBuf(host=x), guard.out_guard(2, n)
    try:
        L.ggml_hip_layer_norm(xb.ptr, n, 2, None, None, out.ptr)
        L.ggml_hip_synchronize()
        y = out.check()
    finally:
        xb.free()
        out.free()
    assert (y.view(np.uint32) == guard.NAN_BITS).all()
    assert "nothing launched" in capfd.readouterr().err
