"""CPU: which kernel form a quantized mat-mul takes. ggllm.cpp_amd/csrc/fq_mm_forms.h -- what fq_launch_gemm, the fq_mul_mat_q_acts family and launch_stage
decide from -- is host-compiled with g++ (tests/host/mm_forms_harness.cpp, default switches) and pinned against tables written out by hand from the rules as
the launchers had them before the header existed: a tile is 32 rows x 32 columns, four partial sums per row below 4 x #CU tiles and two from there on, the
streaming forms up to 32 columns (the k-quants at model widths: 80 / 112), 64-row workgroups from the rb threshold on.

Matrices are named by their number of 32-row tile rows R = ceil(M / 32); n_cu = 256 unless a test says otherwise."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q2_K, Q3_K, Q4_K, Q5_K, Q6_K = 2, 3, 6, 7, 8, 10, 11, 12, 13, 14
LEGACY = (Q4_0, Q4_1, Q5_0, Q5_1, Q8_0)
KQ_A, KQ_B, KQ_C = (Q4_K, Q5_K), (Q2_K, Q3_K), (Q6_K,)      # 80 columns + the 8 x #CU rule / 112 columns / 80 columns
F16, REF, KQREF, GEMV, STREAM, TILE = range(6)
SK_RES, SK_KSHARE, SK_PLAIN, SK_KQ = 1, 2, 3, 4

# (rows, K) of Wqkv, Wo, Wup, Wdown, lm_head
MODELS = {
    "7b":      [(4672, 4544), (4544, 4544), (18176, 4544), (4544, 18176), (65024, 4544)],       # 71 / 1 heads
    "40b":     [(9216, 8192), (8192, 8192), (32768, 8192), (8192, 32768), (65024, 8192)],       # 128 / 8 heads
    "7b-like": [(4864, 4608), (4608, 4608), (18432, 4608), (4608, 18432), (512, 4608)],         # tests/test_gpu_configs.py HP_7B_K: 72 / 2 heads, n_vocab 512
}
ALL_N = [1, 2, 4, 5, 16, 17, 32, 33, 64, 80, 81, 112, 113, 128, 129, 256, 384, 512]

# ---- the tile GEMM's cfg by tile rows R, default order. cfg: 1 = <4,1>, 2 = <4,4>, 3 = <2,4>, 4 = <4,2>, 6 = <2,4,2>
TILE_N = [33, 64, 80, 81, 112, 113, 128, 129, 256, 384, 512]
LEGACY_CFG = {          # legacy formats: every N of TILE_N is a tile launch
    16:   [4, 4, 2, 2, 2, 2, 2, 2, 2, 2, 2],
    142:  [4, 4, 2, 2, 2, 2, 2, 2, 6, 6, 6],
    144:  [4, 4, 2, 2, 2, 2, 2, 2, 6, 6, 6],
    146:  [4, 4, 2, 2, 2, 2, 2, 2, 6, 6, 6],
    152:  [4, 4, 2, 2, 2, 2, 2, 2, 6, 6, 6],
    256:  [4, 4, 2, 2, 3, 3, 3, 3, 6, 6, 6],
    288:  [4, 4, 2, 2, 3, 3, 3, 3, 6, 6, 6],
    568:  [3, 3, 3, 3, 3, 3, 3, 3, 6, 6, 6],
    576:  [3, 3, 3, 3, 3, 3, 3, 3, 6, 6, 6],
    1024: [3, 3, 3, 3, 6, 6, 6, 3, 6, 6, 6],      # 97..128 tokens: 512 64-row workgroups fill the chip twice over (Falcon-40B's Wup)
    2032: [3, 3, 3, 3, 6, 6, 6, 6, 6, 6, 6],
}
KQ_TILE_N = {"A": [81, 112, 113, 128, 129, 256, 384, 512], "B": [113, 128, 129, 256, 384, 512], "C": [81, 112, 113, 128, 129, 256, 384, 512]}
KQ_CFG = {
    "A": {16: [2] * 8, 142: [2, 2, 2, 2, 2, 3, 3, 6], 144: [2, 2, 2, 2, 2, 3, 3, 6], 152: [2, 2, 2, 2, 2, 3, 3, 6], 256: [2, 3, 3, 3, 3, 6, 3, 6],
          288: [2, 3, 3, 3, 3, 6, 3, 6], 576: [3, 6, 6, 6, 6, 6, 3, 6], 1024: [6] * 8, 2032: [6] * 8},
    "B": {16: [2] * 6, 142: [2, 2, 2, 3, 3, 6], 144: [2, 2, 2, 3, 3, 6], 152: [2, 2, 2, 3, 3, 6], 256: [3, 3, 3, 3, 3, 6], 288: [3, 3, 3, 3, 3, 6],
          576: [3, 3, 3, 3, 3, 6], 1024: [3, 3, 3, 6, 6, 6], 2032: [3, 3, 6, 6, 6, 6]},
    "C": {16: [2] * 8, 142: [2, 2, 2, 2, 2, 3, 3, 6], 144: [2, 2, 2, 2, 2, 3, 3, 6], 152: [2, 2, 2, 2, 2, 3, 3, 6], 256: [2, 3, 3, 3, 3, 3, 3, 6],
          288: [2, 3, 3, 3, 3, 3, 3, 6], 576: [3, 3, 3, 3, 3, 3, 3, 6], 1024: [3, 3, 3, 3, 3, 6, 6, 6], 2032: [3, 3, 3, 3, 6, 6, 6, 6]},
}
# cfg -> (K split, weight rows per workgroup, token-tile width): k_gemm_q<S, TT, RB> is 32 RB rows x 32 TT tokens; 16 = the sequential sum's 16 x 16 tiles
CFG_SHAPE = {0: (1, 32, 128), 1: (4, 32, 32), 2: (4, 32, 128), 3: (2, 32, 128), 4: (4, 32, 64), 5: (2, 32, 64), 6: (2, 64, 128), 7: (4, 64, 128), 16: (1, 32, 128)}


def split(R, N):
    """four partial sums below 4 x 256 tiles, two from there on -- written out again on purpose (as tests/test_gpu_configs.py::gemm_split is)"""
    return 4 if R * ((N + 31) // 32) < 1024 else 2


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mmf") / "libmm_forms_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I", os.path.join(ROOT, "ggllm.cpp_amd", "csrc"),
                           "-o", out, os.path.join(ROOT, "tests", "host", "mm_forms_harness.cpp")])
    L = C.CDLL(out)
    ll, i, ip = C.c_longlong, C.c_int, C.POINTER(C.c_int)
    L.mmf_form.restype, L.mmf_form.argtypes = None, [i, ll, ll, ll, i, i, i, i, i, i, ip]
    L.mmf_tile_cfg.restype, L.mmf_tile_cfg.argtypes = i, [i, ll, ll, i, i, i]
    L.mmf_cfg_shape.restype, L.mmf_cfg_shape.argtypes = None, [i, ip]
    L.mmf_gemm_wgs.restype, L.mmf_gemm_wgs.argtypes = ll, [i, ll, ll, ll, i, i]
    L.mmf_pair_split.restype, L.mmf_pair_split.argtypes = i, [i, ll, ll, ll, ll, i, i, i]
    L.mmf_out2_legacy.restype, L.mmf_out2_legacy.argtypes = i, [i, ll, ll, ll, ll, i, i, i]
    L.mmf_q4k_fused_ok.restype, L.mmf_q4k_fused_ok.argtypes = i, [ll, ll, i, i]
    L.mmf_q4k_fused_passes.restype, L.mmf_q4k_fused_passes.argtypes = i, [i, ll, ll, ll, i, i]
    L.mmf_q4k_shape.restype, L.mmf_q4k_shape.argtypes = i, [i, ll, ll]
    L.mmf_cols_max_n.restype, L.mmf_cols_max_n.argtypes = i, [i, ll, ll]
    L.mmf_par2_clash.restype, L.mmf_par2_clash.argtypes = i, [i, ll, ll, ll, ll, i]
    return L


class Form:
    def __init__(self, o):
        self.family, self.S, self.cfg, self.passes, self.pass_w, self.wg_rows, self.tile_cols, self.kind, self.scratch = list(o)

    def __repr__(self):
        return f"Form(family {self.family}, S {self.S}, cfg {self.cfg}, {self.passes} x {self.pass_w} columns, {self.wg_rows} x {self.tile_cols}, kind {self.kind}, scratch {self.scratch})"


def form(H, t, M, K, N, n_cu=256, ref=0, seq=None, force_gemv=0, cfg=-1, from3=0):
    o = (C.c_int * 9)()
    H.mmf_form(t, M, K, N, n_cu, ref, int(ref != 0) if seq is None else seq, force_gemv, cfg, from3, o)
    f = Form(o)
    # ADVICE.md's fifth finding: rows per workgroup and the token-tile width are those of the cfg of the same call
    if f.family == TILE:
        assert (f.S, f.wg_rows, f.tile_cols) == CFG_SHAPE[f.cfg], (t, M, K, N, f)
    elif f.family == STREAM:
        assert (f.wg_rows, f.tile_cols, f.cfg) == (32, 16, -1) and f.passes == (N + 15) // 16, (t, M, K, N, f)
    return f


def kq_class(t):
    return "A" if t in KQ_A else ("B" if t in KQ_B else "C")


def test_cfg_table(H):
    for cfg, want in CFG_SHAPE.items():
        o = (C.c_int * 3)()
        H.mmf_cfg_shape(cfg, o)
        assert tuple(o) == want, cfg


@pytest.mark.parametrize("model", sorted(MODELS))
@pytest.mark.parametrize("t", LEGACY)
def test_default_order_legacy(H, model, t):
    for M, K in MODELS[model]:
        R = (M + 31) // 32
        for N in ALL_N:
            f = form(H, t, M, K, N)
            if N <= 4:
                assert (f.family, f.passes, f.pass_w) == (GEMV, 1, N), (M, K, N, f)
            elif N <= 32:           # the last N of the streaming forms is 32, in passes of 16
                assert (f.family, f.S, f.passes, f.pass_w) == (STREAM, split(R, N), 1 if N <= 16 else 2, min(N, 16)), (M, K, N, f)
                assert f.scratch == (f.kind == SK_KSHARE)
            else:
                assert (f.family, f.cfg) == (TILE, LEGACY_CFG[R][TILE_N.index(N)]), (M, K, N, f)
                assert f.S == split(R, N) and not f.scratch


@pytest.mark.parametrize("model", sorted(MODELS))
@pytest.mark.parametrize("t", KQ_A + KQ_B + KQ_C)
def test_default_order_kquants(H, model, t):
    cls = kq_class(t)
    last = 112 if cls == "B" else 80
    for M, K in MODELS[model]:
        if K % 256:
            continue                # (Falcon-7B's 4544 holds no 256-element super-blocks: only its Wdown is a k-quant matrix)
        R = (M + 31) // 32
        assert H.mmf_q4k_shape(t, M, K) == 1
        for N in ALL_N:
            f = form(H, t, M, K, N)
            if N <= 4:
                assert (f.family, f.passes) == (GEMV, 1), (M, K, N, f)
            elif N <= last:
                assert (f.family, f.S, f.kind, f.scratch) == (STREAM, split(R, N), SK_KQ, 1), (M, K, N, f)
            else:
                assert (f.family, f.cfg) == (TILE, KQ_CFG[cls][R][KQ_TILE_N[cls].index(N)]), (M, K, N, f)
        # lock-step contexts (fq_mul_mat_q_acts_from3): the streaming form from 3 sequences up, 2 keep the mat-vec
        assert form(H, t, M, K, 2, from3=1).family == GEMV
        for N in (3, 4):
            f = form(H, t, M, K, N, from3=1)
            assert (f.family, f.S, f.passes, f.kind) == (STREAM, split(R, N), 1, SK_KQ)


def test_stream_kinds_q4_0(H):
    """which of the legacy streaming forms: the resident columns where they fit LDS (K up to ~4.6 k), the K-share form for long rows at four partial sums"""
    want = {"7b": [SK_RES, SK_RES, SK_RES, SK_KSHARE, SK_RES], "40b": [SK_KSHARE, SK_KSHARE, SK_PLAIN, SK_PLAIN, SK_PLAIN]}
    for model, kinds in want.items():
        for (M, K), kind in zip(MODELS[model], kinds):
            for N in (5, 16, 20, 32):
                assert form(H, Q4_0, M, K, N).kind == kind, (model, M, K, N)


REDUCED_N = [1, 2, 4, 5, 16, 17, 32, 33, 128, 129, 256]


@pytest.mark.parametrize("t", LEGACY + KQ_A + KQ_B + KQ_C)
def test_sequential_and_reference_orders(H, t):
    legacy = t in LEGACY
    for M, K in MODELS["40b"] + MODELS["7b-like"]:
        for N in REDUCED_N:
            # ggml_hip_gemm_sequential alone: the default routes, one left-to-right sum per row
            f = form(H, t, M, K, N, ref=0, seq=1)
            if N <= 4:
                assert f.family == GEMV
            elif legacy and N <= 32:
                assert (f.family, f.S, f.scratch) == (STREAM, 1, 0), (M, K, N, f)
            else:                   # legacy: the 16 x 16 tiles' form up to one tile row of tokens; the k-quants have no streaming form at S = 1
                assert (f.family, f.cfg, f.S) == (TILE, 16 if legacy and N <= 128 else 0, 1), (M, K, N, f)
            # reference order 1: one thread per output, every N
            assert form(H, t, M, K, N, ref=1).family == REF
            # reference order 2: the legacy formats' batches (from two columns) through the S = 1 GEMM side, everything else column by column
            f = form(H, t, M, K, N, ref=2)
            if not legacy or N == 1:
                assert (f.family, f.passes, f.pass_w) == (KQREF, N, 1), (M, K, N, f)
            elif N <= 32:
                assert (f.family, f.S) == (STREAM, 1), (M, K, N, f)
            else:
                assert (f.family, f.cfg) == (TILE, 16 if N <= 128 else 0), (M, K, N, f)


def test_forced_cfg(H):
    """FQ_GEMM_CFG: every GEMM-side launch is that tile cfg, rows per workgroup follow it, and the paired / fused forms step aside"""
    for t in (Q4_0, Q5_1, Q4_K, Q2_K):
        for cfg in (0, 1, 3, 6, 7):
            for N in (5, 16, 20, 128, 512):
                f = form(H, t, 8192, 8192, N, cfg=cfg)
                want = 16 if (cfg == 0 and t in LEGACY and N <= 128) else cfg
                assert (f.family, f.cfg) == (TILE, want), (t, cfg, N, f)
                assert (f.S, f.wg_rows, f.tile_cols) == CFG_SHAPE[want]
    assert H.mmf_gemm_wgs(Q4_0, 4544, 18176, 128, 256, -1) == 142 and H.mmf_gemm_wgs(Q4_0, 4544, 18176, 128, 256, 6) == 71
    assert H.mmf_pair_split(Q4_0, 4672, 18176, 4544, 8, 256, 0, -1) == 4 and H.mmf_pair_split(Q4_0, 4672, 18176, 4544, 8, 256, 0, 2) == 0
    assert H.mmf_out2_legacy(Q4_0, 4544, 4544, 18176, 8, 256, 0, -1) == 1 and H.mmf_out2_legacy(Q4_0, 4544, 4544, 18176, 8, 256, 0, 2) == 0
    assert H.mmf_q4k_fused_ok(8, 5, 0, -1) == 1 and H.mmf_q4k_fused_ok(8, 5, 0, 2) == 0
    assert H.mmf_q4k_fused_passes(Q4_K, 8192, 8192, 48, 0, -1) == 1 and H.mmf_q4k_fused_passes(Q4_K, 8192, 8192, 48, 0, 2) == 0


def test_paired_and_fused_forms(H):
    qkv, up, E, FF = 4672, 18176, 4544, 18176
    # Wqkv + Wup behind one LayerNorm image (Falcon-7B): 5..32 columns, the resident form's K split
    assert [H.mmf_pair_split(Q4_0, qkv, up, E, N, 256, 0, -1) for N in (4, 5, 16, 17, 32, 33)] == [0, 4, 4, 4, 4, 0]
    assert H.mmf_pair_split(Q4_0, qkv, up, E, 8, 256, 1, -1) == 0 and H.mmf_pair_split(Q4_0, qkv, up, E, 8, 256, 2, -1) == 0
    assert H.mmf_pair_split(Q4_0, 9216, 32768, 8192, 8, 256, 0, -1) == 0        # Falcon-40B: four partial sums against two (and the columns do not fit)
    # Wo + Wdown in one K-share launch: Falcon-7B yes, Falcon-40B's Wdown does not fit LDS
    assert [H.mmf_out2_legacy(Q4_0, E, E, FF, N, 256, 0, -1) for N in (4, 5, 16, 17, 32, 33)] == [0, 1, 1, 1, 1, 0]
    assert H.mmf_out2_legacy(Q4_0, 8192, 8192, 32768, 8, 256, 0, -1) == 0
    assert H.mmf_out2_legacy(Q4_0, E, E, FF, 8, 256, 2, -1) == 0
    # the k-quants' fused sum launches: 5..16 columns (lock-step: from 3), passes of 16 up to the type's streaming limit
    assert [H.mmf_q4k_fused_ok(N, 5, 0, -1) for N in (3, 4, 5, 16, 17)] == [0, 0, 1, 1, 0]
    assert [H.mmf_q4k_fused_ok(N, 3, 0, -1) for N in (2, 3, 4)] == [0, 1, 1]
    assert H.mmf_q4k_fused_ok(8, 5, 1, -1) == 0 and H.mmf_q4k_fused_ok(8, 5, 2, -1) == 0
    assert [H.mmf_q4k_fused_passes(Q4_K, 8192, 8192, N, 0, -1) for N in (16, 17, 80, 81)] == [0, 1, 1, 0]
    assert [H.mmf_q4k_fused_passes(Q2_K, 8192, 8192, N, 0, -1) for N in (80, 112, 113)] == [1, 1, 0]


def test_column_limit(H):
    """lock-step contexts of up to this many sequences take the column mat-vec kernels"""
    assert all(H.mmf_cols_max_n(t, 4672, 4544) == 4 for t in LEGACY)
    assert all(H.mmf_cols_max_n(t, 9216, 8192) == 2 for t in KQ_A + KQ_B + KQ_C)           # model widths: the streaming forms from 3 sequences up
    assert H.mmf_q4k_shape(Q4_K, 9208, 8192) == 0 and H.mmf_cols_max_n(Q4_K, 9208, 8192) == 12      # (rows no multiple of 16: only the tile GEMM beyond)


def block(hp):
    return hp["n_embd"], (hp["n_head"] + 2 * hp["n_head_kv"]) * 64, hp["n_ff"]


def test_two_stream_form_and_the_shared_scratch(H):
    """The legacy K-share form keeps its partial sums in ONE process-wide scratch: a block whose main-stream branch (Wqkv, Wo) and side-stream branch (Wup, Wdown)
    would both take it at N columns must not fork (ADVICE.md's first finding)."""
    f7 = block(dict(n_embd=4544, n_head=71, n_head_kv=1, n_ff=18176))
    f40 = block(dict(n_embd=8192, n_head=128, n_head_kv=8, n_ff=32768))
    odd = block(dict(n_embd=8192, n_head=128, n_head_kv=8, n_ff=16384))
    for t in LEGACY:
        for N in list(range(17, 33)) + [33, 64, 128, 512]:
            assert H.mmf_par2_clash(t, *f7, N, 256) == 0, (t, N)         # Falcon-7B: only Wdown takes the K-share form
            assert H.mmf_par2_clash(t, *f40, N, 256) == 0, (t, N)        # Falcon-40B at 256 CUs: Wup sits at 4 x #CU tiles (two partial sums), Wdown does not fit LDS
    # the non-standard width: Wqkv, Wo, Wup (and Wdown) all take it at 17..32 columns
    assert form(H, Q4_0, 16384, 8192, 20).kind == SK_KSHARE and form(H, Q4_0, 9216, 8192, 20).kind == SK_KSHARE
    for t in (Q4_0, Q5_1):
        assert [H.mmf_par2_clash(t, *odd, N, 256) for N in (17, 20, 32, 33)] == [1, 1, 1, 0], t
    # more than 256 CUs: Falcon-40B's Wup falls below 4 x #CU tiles, takes four partial sums and the K-share form, beside Wqkv on the other stream
    assert form(H, Q4_0, 32768, 8192, 20, n_cu=304).kind == SK_KSHARE and form(H, Q4_0, 32768, 8192, 20, n_cu=256).kind == SK_PLAIN
    assert H.mmf_par2_clash(Q4_0, *f40, 20, 304) == 1
    # the k-quants' passes keep a block in stream order by themselves, as before
    assert H.mmf_par2_clash(Q4_K, *f40, 32, 256) == 1 and H.mmf_par2_clash(Q4_K, *f40, 80, 256) == 1 and H.mmf_par2_clash(Q4_K, *f40, 81, 256) == 0
    assert H.mmf_par2_clash(Q2_K, *f40, 112, 256) == 1 and H.mmf_par2_clash(Q2_K, *f40, 113, 256) == 0
