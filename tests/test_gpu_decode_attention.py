"""GPU: the single-token (decode) attention -- attn_head_block<F64, REGS> behind k_attn_decode, k_attn_decode_f64 and k_attn_decode_seqs -- at op level
(ggml_hip_attention_decode) against the oracle's orc_attention_decode, bit for bit, at real head counts and at every boundary of its 128-row register
pipeline up to the single-group LDS limit; the appended cache row, the untouched rest of the caches and the Q8 image with it.
The host-side cases and expected values are tests/decode_attn.py's; tests/test_decode_attn_cases_cpu.py shows on the CPU that they bite."""
import numpy as np
import pytest

import ggllm_cpp_amd as g
import decode_attn as da

pytestmark = pytest.mark.gpu

VARIANTS = [0, 1]            # ggml_hip_reference_order: 0 = f32 FMA chains (oracle order 2), 1 = f64 accumulation (oracle order 0)
LONG_N_PAST, LONG_MAX = 38000, 38400          # attn_decode_lds(n) = 9024 + 4 n <= 160 KiB  =>  n <= 38704


@pytest.fixture(scope="module", autouse=True)
def _init():
    g.init(0)


@pytest.fixture(scope="module")
def tab():
    L = g.load()
    t = L.ggml_hip_rope_table_create(da.D, LONG_MAX, da.ROPE_CTX)
    yield t
    L.ggml_hip_free(t)


class _order:
    def __init__(self, variant):
        self.variant = variant

    def __enter__(self):
        g.load().ggml_hip_reference_order(self.variant)

    def __exit__(self, *a):
        g.load().ggml_hip_reference_order(0)


def _first_diff(got, exp):
    d = np.flatnonzero(got.view(np.uint32) != exp.view(np.uint32))
    return f"{d.size} of {got.size} elements differ, first at {int(d[0])}: {got.flat[d[0]]!r} != {exp.flat[d[0]]!r}" if d.size else ""


def _single(oracle, tab, c, max_n_kv, variant, fill, act_type, seed, at_n_past=None):
    """one single-sequence launch of case c; returns the list of complaints against the oracle, the caches and the image, and the output row"""
    rng = np.random.default_rng(seed)
    kc, vc = da.build_cache(c, max_n_kv, fill, rng, at_n_past)
    with _order(variant):
        att, k_after, v_after, image = da.run_gpu(g, [c], [kc], [vc], 0, max_n_kv, tab, act_type)
    bad = []
    exp = c.expected(oracle, da.ORDER_OF[variant])
    if not np.array_equal(att[0], exp):
        bad.append("output: " + _first_diff(att[0], exp))
    bad += da.check_caches([c], [kc], [vc], k_after, v_after)
    if act_type is not None and not np.array_equal(image, g.quantize_acts(act_type, att)):
        bad.append(f"the {g.TYPE_NAME[act_type]} image is not quantize_acts of the returned row")
    return bad, att[0]


def _b1(oracle, tab, H, HKV, variant, positions):
    failures = []
    for n_past in positions:
        c = da.random_case(oracle, H, HKV, n_past, da.case_seed(H, HKV, n_past))
        for max_n_kv, act_type in ((n_past + 1, g.Q8_0), (da.context_bound(n_past), g.Q8_1)):
            bad, _ = _single(oracle, tab, c, max_n_kv, variant, da.FILL_RANDOM, act_type, seed=n_past + max_n_kv)
            failures += [f"n_past {n_past} (mod 128: {n_past % 128}) max_n_kv {max_n_kv}: {b}" for b in bad]
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("H,HKV", da.HEADS_SMALL)
def test_bit_exact_small_heads(oracle, tab, H, HKV, variant):
    """B1: every position of the list, a plain eval's sizing (max_n_kv = n_past + 1) and a context-sized one (the captured graph's), equal to the oracle
    bit for bit: the default order against oracle order 2 (its association is restated exactly: unconditional), the f64 variant against order 0 (its f64
    partial sums are associated in the kernel's lane order, which moves an f32 result with probability ~1e-9 per dot product: a mismatch is reproducible --
    the seeds are fixed -- and is a kernel bug unless the one differing element is shown, in extended precision, to sit on an f32 rounding boundary)."""
    _b1(oracle, tab, H, HKV, variant, da.N_PAST_ALL)


@pytest.mark.parametrize("H,HKV", da.HEADS_WIDE)
def test_bit_exact_wide_heads(oracle, tab, H, HKV):
    """B1 at Falcon-7B / -40B / -180B head counts, default order"""
    _b1(oracle, tab, H, HKV, 0, da.N_PAST_WIDE)


def test_bit_exact_falcon7b_heads_f64(oracle, tab):
    """B1: the f64 variant at 71 heads (the other wide shapes run the default order only: see test_bit_exact_small_heads on the f64 rule)"""
    _b1(oracle, tab, 71, 1, 1, da.N_PAST_WIDE)


@pytest.mark.parametrize("variant", VARIANTS)
def test_bit_exact_near_the_lds_limit(oracle, tab, variant):
    """B1: 38 000 cached keys under a 38 400-key bound, next to the 38 704 keys one head group's LDS can score"""
    c = da.random_case(oracle, 4, 1, LONG_N_PAST, da.case_seed(4, 1, LONG_N_PAST))
    bad, _ = _single(oracle, tab, c, LONG_MAX, variant, da.FILL_RANDOM, g.Q8_0, seed=3)
    assert not bad, "\n".join(bad)


def test_oversized_bound_is_refused(tab, capfd):
    """a max_n_kv whose score row does not fit the LDS is refused with a message: nothing is launched, nothing is written, the process lives"""
    L = g.load()
    c_qkv = np.zeros((6, 64), np.float32)
    qb, kb, pb, ab = g.DevBuf(host=c_qkv), g.DevBuf(4096), g.DevBuf(host=np.zeros(1, np.int32)), g.DevBuf(4 * 64 * 4)
    L.ggml_hip_memset(ab.ptr, 0xFF, 4 * 64 * 4)
    L.ggml_hip_attention_decode(qb.ptr, 1, 4, 1, pb.ptr, 0, 38705, tab, kb.ptr, kb.ptr, 0, ab.ptr, None, 0)
    L.ggml_hip_synchronize()
    assert np.all(ab.to_host(np.uint32, (4 * 64,)) == 0xFFFFFFFF)
    assert "do not fit" in capfd.readouterr().err
    for b in (qb, kb, pb, ab):
        b.free()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("H,HKV", [(71, 1), (128, 8)])
def test_rows_past_the_end_do_not_matter(oracle, tab, H, HKV, variant):
    """B2: the same call with cache rows (n_past, max_n_kv) holding zeros, +-3.0e38 and random values, and row n_past itself (which the kernel overwrites and
    must not read for its scores) holding 3.0e38 before the call: three bit-identical results, equal to the oracle's. FINITE values on purpose: the kernel's
    contract is a clamped, finite re-read multiplied by a zero weight, and the model's caches are zero-filled at creation. One route by which a
    non-finite row can still come to lie past the end of a live sequence (written up in DESIGN.md, section 2): a sequence that overflowed leaves non-finite
    values in its rows, and the context is then reused from position 0 -- the early loads re-read value rows [0, 128), and NaN * 0 is NaN until the new
    sequence has overwritten them. That is outside the contract tested here."""
    failures = []
    for n_past in (0, 5, 127, 128, 130, 255, 300):
        c = da.random_case(oracle, H, HKV, n_past, da.case_seed(H, HKV, n_past, salt=1))
        for max_n_kv in (n_past + 1, da.context_bound(n_past)):
            rows = []
            for fill in (da.FILL_ZERO, da.FILL_HUGE, da.FILL_RANDOM):
                bad, row = _single(oracle, tab, c, max_n_kv, variant, fill, None, seed=n_past, at_n_past=np.float32(3.0e38))
                failures += [f"n_past {n_past} max_n_kv {max_n_kv} fill {fill}: {b}" for b in bad]
                rows.append(row)
            if not (np.array_equal(rows[0], rows[1]) and np.array_equal(rows[0], rows[2])):
                failures.append(f"n_past {n_past} max_n_kv {max_n_kv}: the result depends on rows past the end")
    assert not failures, "\n".join(failures)


def _probe_j_star(n_past, i, HKV):
    tg = da.probe_targets(n_past)
    return [tg[(i + 5 * hk) % len(tg)] for hk in range(HKV)]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("H,HKV", [(71, 1), (8, 2)])
def test_probe_single_sequence(oracle, tab, H, HKV, variant):
    """B3: which key is where. One key per kv head scores 32, all others exactly 0; fp16 exp(-32) is exactly 0, so the output must be value row j* of the
    head's kv head bit for bit, whatever the association -- no oracle involved. j* sweeps the step boundaries, the last cached row and the newest key, each
    kv head with its own j*. A kernel that reads the wrong row, the wrong kv head or a stale register step fails outright."""
    failures = []
    for n_past in da.PROBE_N_PAST:
        for i in range(len(da.probe_targets(n_past))):
            j_star = _probe_j_star(n_past, i, HKV)
            c, exp = da.probe_case(oracle, H, HKV, n_past, j_star, seed=1000 * n_past + i)
            for max_n_kv in (n_past + 1, da.context_bound(n_past)):
                kc, vc = da.build_cache(c, max_n_kv, da.FILL_RANDOM, np.random.default_rng(i))
                with _order(variant):
                    att, k_after, v_after, _ = da.run_gpu(g, [c], [kc], [vc], 0, max_n_kv, tab)
                if not np.array_equal(att[0], exp):
                    failures.append(f"n_past {n_past} j* {j_star} max_n_kv {max_n_kv}: " + _first_diff(att[0], exp))
                failures += [f"n_past {n_past} j* {j_star}: {b}" for b in da.check_caches([c], [kc], [vc], k_after, v_after)]
    assert not failures, "\n".join(failures)


# (k_attn_decode_seqs has ONE arithmetic, f32 chains: there is no f64 ragged path. The run under reference order 1 only guards against the order flag
#  leaking into the seqs launcher -- it must select the same kernel and give the same exact rows.)
@pytest.mark.parametrize("variant", [pytest.param(0, id="default"), pytest.param(1, id="order-flag-must-not-leak")])
@pytest.mark.parametrize("H,HKV", [(71, 1), (8, 2)])
def test_probe_ragged_sequences(oracle, tab, H, HKV, variant):
    """B3 over a ragged launch: five sequences at five different n_past at once, each with its own j* per kv head and its own values -- a kernel that reads
    a neighbour sequence's cache or position fails outright."""
    failures = []
    max_n_kv = 2048
    for i in range(max(len(da.probe_targets(n)) for n in da.PROBE_N_PAST)):
        cases, exps = [], []
        for t, n_past in enumerate(da.PROBE_N_PAST):
            j_star = _probe_j_star(n_past, i + t, HKV)
            c, exp = da.probe_case(oracle, H, HKV, n_past, j_star, seed=77 * n_past + i)
            cases.append(c)
            exps.append(exp)
        rng = np.random.default_rng(i)
        caches = [da.build_cache(c, max_n_kv, da.FILL_RANDOM, rng) for c in cases]
        kcs, vcs = [k for k, _ in caches], [v for _, v in caches]
        with _order(variant):
            att, k_after, v_after, _ = da.run_gpu(g, cases, kcs, vcs, 1, max_n_kv, tab)
        for t, c in enumerate(cases):
            if not np.array_equal(att[t], exps[t]):
                failures.append(f"sweep {i} seq {t} (n_past {c.n_past}): " + _first_diff(att[t], exps[t]))
        failures += [f"sweep {i}: {b}" for b in da.check_caches(cases, kcs, vcs, k_after, v_after)]
    assert not failures, "\n".join(failures)


SPREAD = [0, 2047, 129, 257, 385, 513, 641, 1023, 1024, 127, 128, 255, 256, 384, 512, 640]      # one row at 0, one at max_n_kv - 1


@pytest.mark.parametrize("pos_stride", [0, 1])
@pytest.mark.parametrize("n_seq", [2, 5, 16])
@pytest.mark.parametrize("H,HKV", [(71, 1), (128, 8)])
def test_lockstep_and_ragged_launches(oracle, tab, H, HKV, n_seq, pos_stride):
    """B4: n_seq rows in one k_attn_decode_seqs launch, all at one position (pos_stride 0) or each at its own (1: spread over the boundary list, one row at 0
    and one at max_n_kv - 1): every row equals the oracle and the single-sequence launch of the same inputs, bit for bit, with its Q8 image; only row pos[t]
    of sequence t's caches is written."""
    max_n_kv = 2048
    positions = SPREAD[:n_seq] if pos_stride else [385] * n_seq
    cases = [da.random_case(oracle, H, HKV, p, da.case_seed(H, HKV, p, salt=100 + t)) for t, p in enumerate(positions)]
    rng = np.random.default_rng(n_seq)
    caches = [da.build_cache(c, max_n_kv, da.FILL_RANDOM, rng) for c in cases]
    kcs, vcs = [k for k, _ in caches], [v for _, v in caches]
    act_type = g.Q8_1 if pos_stride else g.Q8_0
    att, k_after, v_after, image = da.run_gpu(g, cases, kcs, vcs, pos_stride, max_n_kv, tab, act_type)
    failures = da.check_caches(cases, kcs, vcs, k_after, v_after)
    if not np.array_equal(image, g.quantize_acts(act_type, att)):
        failures.append("the image is not quantize_acts of the returned rows")
    for t, c in enumerate(cases):
        exp = c.expected(oracle, 2)
        if not np.array_equal(att[t], exp):
            failures.append(f"seq {t} (n_past {c.n_past}) vs the oracle: " + _first_diff(att[t], exp))
        one, _, _, _ = da.run_gpu(g, [c], [kcs[t]], [vcs[t]], 0, max_n_kv, tab)
        if not np.array_equal(att[t], one[0]):
            failures.append(f"seq {t} (n_past {c.n_past}) vs the single-sequence launch: " + _first_diff(att[t], one[0]))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("H,HKV,n_past", [(4, 1, 8191), (8, 2, 4095), (71, 1, 2047), (128, 8, 513), (232, 8, 513)])
def test_against_plain_numpy_f64(oracle, tab, H, HKV, n_past):
    """B5, a second witness that shares nothing with the oracle's C code but the soft_max: the numpy f64 restatement test_attention uses, under that
    test's own bounds (2e-6 for the f64 variant, 2e-3 for the default order's f32 chains)"""
    c = da.random_case(oracle, H, HKV, n_past, da.case_seed(H, HKV, n_past))
    exp = da.attention_ref(oracle, c.q_rot[None], c.keys(), c.values(), n_past, H, HKV)[0]

    def relrms(a, b):
        return float(np.abs(a.astype(np.float64) - b).max() / (np.sqrt((b.astype(np.float64) ** 2).mean()) + 1e-30))
    max_n_kv = da.context_bound(n_past)
    kc, vc = da.build_cache(c, max_n_kv, da.FILL_RANDOM, np.random.default_rng(1))
    got = {}
    for variant in VARIANTS:
        with _order(variant):
            got[variant] = da.run_gpu(g, [c], [kc], [vc], 0, max_n_kv, tab)[0][0]
    print("decode attention vs numpy f64:", relrms(got[1], exp), relrms(got[0], exp))
    assert relrms(got[1], exp) <= 2e-6, relrms(got[1], exp)
    assert relrms(got[0], exp) <= 2e-3, relrms(got[0], exp)
