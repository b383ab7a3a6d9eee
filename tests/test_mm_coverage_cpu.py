"""CPU: every mat-mul launch the Falcon-7B / 40B / 180B matrices take at 5..129 columns is one the op-level GPU tests run.

csrc/fq_mm_forms.h states, in fq_mm_launch_key, the structural facts of a launch -- family, K split S, passes, streaming form, weight stages NBW, tiles per
workgroup, whether workgroups loop or walk, ragged tails -- from the plan functions the launchers call. This test host-compiles it (tests/mm_keys.py: tests/host/
mm_forms_harness.cpp, default switches, 256 CUs), takes the keys of the model matrices (production) and of the shapes in tests/mm_shapes.py (tested: what
tests/test_gpu_mul_mat.py and tests/test_gpu_op_contract.py parametrize from) and asserts production <= tested. A key is taken per format: the kernels are
instantiated per format. The new GPU cases assert in turn that the device plans the key computed here (ggml_hip_debug_mul_mat_plan), so a chip with another CU
count fails there instead of testing another form."""
import mm_shapes as ms
from mm_keys import key as _key, STREAM, TILE, SK_RES, SK_KSHARE, SK_PLAIN, SK_KQ
from mm_shapes import Q4_0, Q4_1, Q5_1, Q8_0

key = _key

# (rows, K) of Wqkv, Wo, Wup, Wdown, lm_head (vocabulary 65 024)
MODELS = {
    "7b":   [(4672, 4544), (4544, 4544), (18176, 4544), (4544, 18176), (65024, 4544)],           # 71 / 1 heads
    "40b":  [(9216, 8192), (8192, 8192), (32768, 8192), (8192, 32768), (65024, 8192)],           # 128 / 8 heads
    "180b": [(15872, 14848), (14848, 14848), (59392, 14848), (14848, 59392), (65024, 14848)],    # 232 / 8 heads
}
ALL_N = [1, 2, 4, 5, 16, 17, 32, 33, 64, 80, 81, 112, 113, 128, 129, 256, 384, 512]                 # tests/test_mm_forms_cpu.py
PRODUCTION_N = list(range(5, 34)) + [n for n in ALL_N if 33 < n <= 129]
CFG_ROWS_COLS = {0: (32, 128), 1: (32, 32), 2: (32, 128), 3: (32, 128), 4: (32, 64), 5: (32, 64), 6: (64, 128), 7: (64, 128), 16: (32, 128)}      # tests/test_mm_forms_cpu.py CFG_SHAPE


def production():
    """key -> the first (model, matrix, type, K, M, N, mode, from3) that takes it"""
    keys = {}
    for model, mats in MODELS.items():
        for name, (M, K) in zip(("Wqkv", "Wo", "Wup", "Wdown", "lm_head"), mats):
            for t in ms.WEIGHT_TYPES:
                if K % ms.BLCK[t]:
                    continue                # (Falcon-7B's 4544 holds no 256-element super-blocks)
                for mode in ("default", "seq"):
                    for N in PRODUCTION_N:
                        keys.setdefault(key(t, K, M, N, mode), (model, name, t, K, M, N, mode, 0))
                if t in ms.KQUANTS:
                    for N in (3, 4):        # lock-step contexts of 3 and 4 sequences (fq_mul_mat_q_acts_from3)
                        keys.setdefault(key(t, K, M, N, from3=1), (model, name, t, K, M, N, "default", 1))
    return keys


def reached(k, M, N):
    """the keys a launch with key k reaches: its own and, where it has whole row units ahead of a ragged last one (whole column tiles ahead of a ragged last
    one), that of the same launch without the tail -- the whole units of a ragged matrix run what every unit of an even one runs, the ragged unit runs the
    masked path on top. Never the other way round: an even shape does not count for a ragged one."""
    t, fam, S, multi, kind, a, b, c, d = k
    out = {k}
    if fam == TILE:
        rows, cols = CFG_ROWS_COLS[a]
        for cc in {c, 0 if M > rows else c}:
            for dd in {d, 0 if N > cols else d}:
                out.add((t, fam, S, multi, kind, a, b, cc, dd))
    elif fam == STREAM and kind in (SK_RES, SK_PLAIN) and M > 32:
        out.add((t, fam, S, multi, kind, a, b, 0, d))
    elif fam == STREAM and kind == SK_KSHARE and M > 16:
        out.add((t, fam, S, multi, kind, a, b, c, 0))
    return out


def keys_tested(cases=None):
    out = set()
    for t, K, M, N, mode in (ms.op_level_cases() if cases is None else cases):
        out |= reached(key(t, K, M, N, mode), M, N)
    return out


def describe(k):
    t, fam, S, multi, kind, a, b, c, d = k
    what = {TILE: f"tile cfg {a}, token-tile rows > 1: {b}, ragged rows {c}, ragged columns {d}",
            STREAM: {SK_RES: f"resident, NBW {a}, loop {b}, ragged pair {c}", SK_KSHARE: f"K-share, NBW {a}, T class {b}, walk {c}, ragged tile {d}",
                     SK_PLAIN: f"per-stage, ragged tile {c}", SK_KQ: f"k-quant kernel {a}, several segments {b}, walk {c}, NBW {d}"}.get(kind, "?")}.get(fam, f"family {fam}")
    return f"type {t} S {S} passes > 1: {multi}: {what}"


def missing(cases=None, show=True):
    prod, have = production(), keys_tested(cases)
    miss = sorted(k for k in prod if k not in have)
    if show:
        for k in miss:
            print(f"not reached: {k} ({describe(k)}), taken by {prod[k]}")
    return miss, prod


def test_closure():
    """production <= tested"""
    miss, prod = missing()
    assert not miss, f"{len(miss)} of {len(prod)} launch keys of the model matrices are reached by no op-level GPU shape (listed above)"


def test_closure_needs_the_model_sized_shapes():
    """non-vacuity of the closure: without the shapes this census added, keys of every streaming form and of the tile GEMM are open; and each row of
    MODEL_FORMS_LEGACY alone reaches some key of the model matrices that no other shape reaches"""
    new = set(ms.model_forms_legacy_cases() + ms.model_forms_further_cases() + ms.tile_forms_even_cases())
    miss, prod = missing([c for c in ms.op_level_cases() if c not in new], show=False)
    kinds = {(k[1], k[4]) for k in miss}
    assert {(STREAM, SK_RES), (STREAM, SK_KSHARE), (STREAM, SK_PLAIN), (STREAM, SK_KQ), (TILE, 0)} <= kinds and len(prod) > 200
    idle = []
    for row in ms.MODEL_FORMS_LEGACY + ms.MODEL_FORMS_FURTHER:
        K, M, N, mode, types = row
        drop = {(t, K, M, N, mode) for t in types}
        if not missing([c for c in ms.op_level_cases() if c not in drop], show=False)[0]:
            idle.append(row)
    print("rows that reach no key of the model matrices by themselves:", idle)
    # rows the issue names that share their model-matrix keys with another row, and stay: K = 512 at one pass (NBW 3 for every format: the model widths have it for
    # Q4_0 / Q4_1 only, where (4544, ..) reaches it too), T = 2 and T = 5 (one class, 1 < T < 8), the largest M (the key of (8192, 9216, 5))
    assert set(idle) <= {(512, 32741, 5, "default", ms.LEGACY), (512, 8229, 9, "default", ms.LEGACY), (512, 8229, 9, "seq", ms.LEGACY),
                         (8192, 1040, 5, "default", ms.LEGACY), (8192, 4544, 7, "default", ms.LEGACY), (8192, 32736, 16, "default", (Q4_0,))}, idle


def test_model_form_shapes_land_where_they_say():
    """the shapes of mm_shapes.MODEL_FORMS_LEGACY land in the forms their comments name"""
    def k(K, M, N, mode="default", t=Q4_0):
        return key(t, K, M, N, mode)[1:]

    def but_nbw(kk):
        return kk[:4] + kk[5:]
    for t in ms.LEGACY:
        nbw_7b = 3 if t in (Q4_0, Q4_1) else 2        # 142 blocks beside 16 resident columns
        assert k(512, 32741, 5, t=t) == (STREAM, 2, 0, SK_RES, 3, 1, 1, 0)
        assert k(512, 32741, 17, t=t) == (STREAM, 2, 1, SK_RES, 3, 1, 1, 0)
        assert k(4544, 32741, 5, t=t) == ((STREAM, 2, 0, SK_PLAIN, 0, 0, 1, 0) if t == Q8_0 else (STREAM, 2, 0, SK_RES, nbw_7b, 1, 1, 0))
        assert k(6144, 32741, 5, t=t) == (STREAM, 2, 0, SK_PLAIN, 0, 0, 1, 0)
        assert k(6144, 32741, 17, t=t) == (STREAM, 2, 1, SK_PLAIN, 0, 0, 1, 0)
        assert k(6144, 40, 17, t=t) == (STREAM, 4, 1, SK_PLAIN, 0, 0, 1, 0)
        for mode, S in (("default", 4), ("seq", 1)):
            assert k(512, 8229, 9, mode, t=t) == (STREAM, S, 0, SK_RES, 3, 1, 1, 0)
            assert k(512, 8229, 20, mode, t=t) == (STREAM, S, 1, SK_RES, 3, 1, 1, 0)
            if t != Q8_0:
                assert but_nbw(k(4544, 8229, 16, mode, t=t)) == (STREAM, S, 0, SK_RES, 1, 1, 0)
        if t != Q8_0:
            assert k(4544, 8229, 16, t=t)[4] == (3 if t == Q4_0 else 2)      # (S = 4: three exchange buffers more than at S = 2)
        else:
            assert k(4544, 8229, 16, t=t) == (STREAM, 4, 0, SK_PLAIN, 0, 0, 1, 0)      # (142 Q8_0 blocks beside 16 columns: not resident)
        assert k(8192, 1040, 5, t=t) == (STREAM, 4, 0, SK_KSHARE, 3, 2, 0, 0)
        assert k(8192, 4544, 7, t=t) == (STREAM, 4, 0, SK_KSHARE, 3, 2, 0, 0)
        assert k(18176, 4544, 12, t=t) == (STREAM, 4, 0, SK_KSHARE, 3 if t in (Q4_0, Q4_1) else 2, 2, 0, 0)
        assert but_nbw(k(8192, 8192, 16, t=t)) == (STREAM, 4, 0, SK_KSHARE, 3, 0, 0)
        assert but_nbw(k(8192, 9216, 5, t=t)) == (STREAM, 4, 0, SK_KSHARE, 3, 1, 0)
        assert but_nbw(k(8192, 9216, 29, t=t)) == (STREAM, 4, 1, SK_KSHARE, 3, 1, 0)
    assert k(8192, 32736, 16) == (STREAM, 4, 0, SK_KSHARE, 3, 3, 1, 0)


def test_keys_of_the_model_matrices_by_hand():
    """the keys of four production launches, written out by hand from the launchers' rules (csrc/kernels_gemm_skinny.hip fq_launch_gemm_skinny)"""
    # Falcon-7B lm_head, Q4_0, 8 lock-step sequences: 2032 x 1 tiles >= 4 x 256 -> S = 2. 142 blocks: 3 x 32 rows x 592 B of weight stages + 16 x 4624 B of columns
    # + 2 x 142 x 16 x 4 B of scales + the two shares' exchange (4096 B) = 153 088 B <= 160 KiB -> resident, NBW 3. 2032 row pairs on 256 persistent workgroups:
    # they loop; 65 024 = 2032 x 32: no ragged pair
    assert key(Q4_0, 4544, 65024, 8) == (Q4_0, STREAM, 2, 0, SK_RES, 3, 1, 0, 0)
    # Falcon-40B Wup, Q4_0, 20 columns: 1024 tiles = 4 x 256 -> S = 2. 256 blocks: the columns alone are 16 x 8208 B = 131 328 B, with two weight stages and the
    # scales beyond 160 KiB -> not resident; the K-share form is S = 4's -> the per-stage form k_gemm_skinny<Q4_0, 2>, two passes (16 + 4)
    assert key(Q4_0, 8192, 32768, 20) == (Q4_0, STREAM, 2, 1, SK_PLAIN, 0, 0, 0, 0)
    # Falcon-40B Wqkv, Q5_1, 5 columns: 288 tiles -> S = 4; 256 blocks, 9216 <= 32 768 rows -> the K-share form. 576 16-row tiles x 4 shares / 256 CUs = 9 -> T = 8,
    # 72 row blocks; 72 slots x 4 shares > 256 CUs -> 64 slots: the walk. 9216 = 576 x 16: no ragged tile. A stage of one Q5_1 tile is 6400 B:
    # 3 x 8 x 6400 + 16 x 2064 B (a quarter of the columns) + 8192 B of scales = 194 816 B > 160 KiB, with two stages 143 616 B -> NBW 2
    assert key(Q5_1, 8192, 9216, 5) == (Q5_1, STREAM, 4, 0, SK_KSHARE, 2, 3, 1, 0)
    # Falcon-7B lm_head, Q8_0, 8 columns: S = 2. A row's stage of 32 Q8_0 blocks is 32 x 34 = 1088 B, 1104 with the odd-slot padding; 2 x 32 x 1104 + 73 984 +
    # 18 176 + 4096 = 166 912 B > 160 KiB -> not resident; S = 2 -> not the K-share form: k_gemm_skinny<Q8_0, 2>
    assert key(Q8_0, 4544, 65024, 8) == (Q8_0, STREAM, 2, 0, SK_PLAIN, 0, 0, 0, 0)
    prod = production()
    for k in (key(Q4_0, 4544, 65024, 8), key(Q4_0, 8192, 32768, 20), key(Q5_1, 8192, 9216, 5), key(Q8_0, 4544, 65024, 8)):
        assert k in prod
    # a k-quant and a tile launch, the families the four above do not name. Falcon-40B lm_head, Q4_K, 8 columns: S = 2, 32 super-blocks = one segment; 4064 tiles
    # x 2 share pairs / 256 CUs -> T = 8; three stages of 8 tiles (129 024 B) beside 16 x 4112 B of columns do not fit, two do (162 064 B) -> NBW 2; 508 row blocks
    # on (256 / 2 / 8) x 8 = 128 slots: the workgroups walk.
    # Falcon-7B Wqkv, Q4_1, 80 columns: 146 x 3 tiles -> S = 4, <4, 4> (cfg 2), one 128-token tile row, 4672 = 146 x 32, 80 columns of 128
    assert key(ms.Q4_K, 8192, 65024, 8) == (ms.Q4_K, STREAM, 2, 0, SK_KQ, 1, 0, 1, 2)
    assert key(Q4_1, 4544, 4672, 80) == (Q4_1, TILE, 4, 0, 0, 2, 0, 0, 1)
