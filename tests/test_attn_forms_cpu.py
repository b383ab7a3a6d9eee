"""CPU: which kernel a prompt (prefill) attention launch takes. ggllm.cpp_amd/csrc/fq_attn_forms.h -- what fq_launch_attention launches from and what sizes a
context's scratch -- is host-compiled with g++ (tests/host/attn_forms_harness.cpp; default switches unless a test names others, never the environment's) and pinned
against tables written out by hand from the launcher's if-chain as it stood before the header existed:

  score row = ((n_kv + 3) & ~3) floats; the rows forms keep 8256 bytes of reduction space in front of them; 4 rows while 8256 + 4 row <= 56 KiB, else 2 while
  8256 + 2 row <= 150 KiB (and then, from 4 tokens on, 4 rows on the global scratch), else 1; refusal beyond 160 KiB for one row.
  From 32 tokens on, default order: k_attention_flash at pitch 16 / 32 / 64 / 74 key tiles, its LONG form beyond 74.

n_kv below is the launch's largest (n_past + N); n_cu = 256 unless a test says otherwise."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REFUSE_D, REFUSE_KEYS, ONE, ROWS, ROWS_SCRATCH, FLASH, MFMA16, MFMA16H, MFMA_SCRATCH = range(9)      # fq_attn_family (FQ_AF_*)
SW_NAMES = ["rows", "mfma", "mfma16", "mfma16h", "mfma16_maxkv", "flash", "flash_long", "flash_tab", "keep", "persist", "pack_min_n", "scratch", "scratch_gb", "dbg"]
SW_DEFAULT = dict(rows=-1, mfma=1, mfma16=0, mfma16h=0, mfma16_maxkv=4096, flash=1, flash_long=1, flash_tab=1, keep=1, persist=1, pack_min_n=256, scratch=1,
                  scratch_gb=4, dbg=0)
KiB, MiB, GiB = 1 << 10, 1 << 20, 1 << 30


@pytest.fixture(scope="module")
def A(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("atf") / "libattn_forms_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I", os.path.join(ROOT, "ggllm.cpp_amd", "csrc"),
                           "-o", out, os.path.join(ROOT, "tests", "host", "attn_forms_harness.cpp")])
    L = C.CDLL(out)
    i, ll, ip, lp = C.c_int, C.c_longlong, C.POINTER(C.c_int), C.POINTER(C.c_longlong)
    L.atf_default_switches.restype, L.atf_default_switches.argtypes = None, [ip]
    L.atf_plan.restype, L.atf_plan.argtypes = None, [i, i, i, i, i, i, i, i, ip, i, ll, lp]
    L.atf_scratch_need.restype, L.atf_scratch_need.argtypes = ll, [i, i, i, i, ip]
    L.atf_one_row_lds.restype, L.atf_one_row_lds.argtypes = ll, [i]
    L.atf_one_row_fits.restype, L.atf_one_row_fits.argtypes = i, [i]
    return L


def sw_arr(sw):
    assert not set(sw) - set(SW_DEFAULT), sw
    return (C.c_int * 14)(*[dict(SW_DEFAULT, **sw)[k] for k in SW_NAMES])


class Plan:
    def __init__(self, o):
        (self.family, self.R, self.nt, self.keep, self.long, self.packed, self.nt_total, self.ctx_tab, self.persistent, self.gx, self.gy, self.block, self.lds,
         self.pitch, self.scratch, self.dbg) = list(o)

    def __repr__(self):
        return (f"Plan(family {self.family}, R {self.R}, nt {self.nt} keep {self.keep} long {self.long}, packed {self.packed}, persistent {self.persistent}, "
                f"grid {self.gx} x {self.gy} x {self.block}, lds {self.lds}, pitch {self.pitch}, scratch {self.scratch})")


def plan(A, N, n_past, H=2, HKV=1, D=64, lockstep=0, f64=0, form=0, n_cu=256, cap=-1, **sw):
    o = (C.c_longlong * 16)()
    A.atf_plan(N, H, HKV, D, n_past + N, lockstep, f64, form, sw_arr(sw), n_cu, cap, o)
    return Plan(o)


def row_bytes(n_kv):
    return ((n_kv + 3) & ~3) * 4


def test_default_switches(A):
    v = (C.c_int * 14)()
    A.atf_default_switches(v)
    assert dict(zip(SW_NAMES, v)) == SW_DEFAULT


def test_anchors(A):
    """a handful of shapes read off the chain one by one (tests/test_gpu_block_ops.py's own shapes among them)"""
    p = plan(A, 5, 37)
    assert (p.family, p.R, p.gx, p.gy, p.block, p.lds, p.scratch) == (ROWS, 4, 2, 2, 256, 8256 + 4 * 4 * 44, 0), p
    p = plan(A, 6, 3500)                    # two rows fit -> four on the scratch
    assert (p.family, p.R, p.gy, p.lds, p.pitch, p.scratch) == (ROWS_SCRATCH, 4, 2, 8256, 3508, 2 * 2 * 4 * 14032), p
    p = plan(A, 2, 20000)
    assert (p.family, p.R, p.gy, p.lds) == (ONE, 1, 2, 88272), p
    p = plan(A, 40, 3000, f64=1)            # 8256 + 4 x 12160 = 56896 <= 57344
    assert (p.family, p.R, p.gy, p.lds) == (ROWS, 4, 10, 56896), p
    p = plan(A, 512, 7680)
    assert (p.family, p.nt, p.keep, p.long, p.packed, p.nt_total, p.scratch, p.lds, p.block) == (FLASH, 64, 0, 1, 1, 256, 256 * 16384, 142864, 512), p
    p = plan(A, 33, 2400)
    assert (p.family, p.nt, p.keep, p.long, p.packed, p.nt_total, p.scratch) == (FLASH, 64, 0, 1, 0, 0, 0), p
    p = plan(A, 70, 2290)                   # 2360 keys = 74 tiles
    assert (p.family, p.nt, p.keep, p.long, p.lds) == (FLASH, 74, 0, 0, 163344), p
    # (70 tokens behind 2390 -- test_prefill_attention_forms_are_bit_identical's last shape -- are 2460 keys = 77 tiles: the chain's attn_flash_nt gives the LONG form
    # there, not pitch 74)
    p = plan(A, 70, 2390)
    assert (p.family, p.nt, p.keep, p.long) == (FLASH, 64, 0, 1), p


def test_refusals(A):
    assert plan(A, 5, 37, D=128).family == REFUSE_D and plan(A, 5, 37, D=32).family == REFUSE_D
    # one row: 8256 + row <= 160 KiB = 163840 -> 38896 keys at the most
    assert plan(A, 1, 38895).family == ONE and plan(A, 1, 38895).lds == 160 * KiB
    for N, kw in ((1, {}), (4, {}), (512, {}), (512, dict(form=32)), (3, dict(lockstep=1)), (64, dict(f64=1))):
        assert plan(A, N, 38897 - N, **kw).family == REFUSE_KEYS, (N, kw)
        assert plan(A, N, 38896 - N, **kw).family != REFUSE_KEYS, (N, kw)
    assert plan(A, 5, 50000, D=65).family == REFUSE_D            # head_dim is looked at first
    assert A.atf_one_row_fits(38896) == 1 and A.atf_one_row_fits(38897) == 0
    assert [A.atf_one_row_lds(n) for n in (1, 4, 5, 2048)] == [8272, 8272, 8288, 8256 + 8192]       # the verify pair's LDS bytes


def test_one_two_or_four_rows(A):
    """below 32 tokens (and in f64 order at any N): 4 rows while 8256 + 4 row <= 56 KiB (3068 keys), 2 rows while 8256 + 2 row <= 150 KiB (18168 keys) -- and then
    four on the scratch from 4 tokens on --, else one"""
    for f64 in (0, 1):
        for N, want in ((1, (ONE, 1)), (2, (ROWS, 2)), (3, (ROWS, 2)), (4, (ROWS, 4)), (31, (ROWS, 4))):
            p = plan(A, N, 100, f64=f64)
            assert (p.family, p.R) == want and p.gy == (N + p.R - 1) // p.R and p.lds == 8256 + p.R * row_bytes(100 + N) and p.scratch == 0, (N, p)
        # the 56 KiB boundary
        assert 8256 + 4 * row_bytes(3068) == 56 * KiB
        p = plan(A, 8, 3060, f64=f64)
        assert (p.family, p.R, p.lds) == (ROWS, 4, 56 * KiB), p
        p = plan(A, 8, 3061, f64=f64)
        assert (p.family, p.R, p.lds, p.pitch, p.scratch) == (ROWS_SCRATCH, 4, 8256, 3072, 2 * 2 * 4 * 4 * 3072), p
        for N in (2, 3):                    # fewer than 4 tokens: two rows in LDS
            p = plan(A, N, 3069 - N, f64=f64)
            assert (p.family, p.R, p.lds) == (ROWS, 2, 8256 + 2 * 4 * 3072), p
        # the 150 KiB boundary: 8256 + 2 x 4 x 18168 = 153600
        p = plan(A, 2, 18166, f64=f64)
        assert (p.family, p.R, p.lds) == (ROWS, 2, 150 * KiB), p
        p = plan(A, 2, 18167, f64=f64)
        assert (p.family, p.R, p.gy, p.lds) == (ONE, 1, 2, 8256 + 4 * 18172), p
        assert plan(A, 8, 18160, f64=f64).family == ROWS_SCRATCH
        p = plan(A, 8, 18161, f64=f64)      # two rows do not fit: no scratch form either
        assert (p.family, p.R, p.gy) == (ONE, 1, 8), p
    # f64: never the matrix pipe, whatever the form
    for form in (0, 1, 16, 17, 32):
        p = plan(A, 512, 0, f64=1, form=form)
        assert (p.family, p.R, p.gy) == (ROWS, 4, 128), p
        assert plan(A, 512, 7680, f64=1, form=form, H=71).family == ROWS_SCRATCH


def test_lockstep_is_always_one_row(A):
    for N in (1, 2, 4, 31, 32, 64, 512):
        for kw in ({}, dict(f64=1), dict(form=32), dict(rows=8), dict(rows=4), dict(mfma=0)):
            for n_past in (0, 3500):
                p = plan(A, N, n_past, H=71, lockstep=1, **kw)
                assert (p.family, p.R, p.gx, p.gy, p.block, p.lds, p.scratch) == (ONE, 1, 71, N, 256, 8256 + row_bytes(n_past + N), 0), (N, kw, p)


FLASH_LDS = {16: 44560, 32: 77328, 64: 142864, 74: 163344}      # 32 x (32 nt + 8) x 2 + 1024 + 2048 + 8192 + 16


def test_flash_pitches(A):
    """from 32 tokens on: 16 / 32 / 64 key tiles with the scores kept in registers, 65..74 tiles at pitch 74 without, the LONG form (chunks of 64 tiles) beyond"""
    table = [(1, 16, 1, 0), (512, 16, 1, 0), (513, 32, 1, 0), (1024, 32, 1, 0), (1025, 64, 1, 0), (2048, 64, 1, 0), (2049, 74, 0, 0), (2368, 74, 0, 0),
             (2369, 64, 0, 1), (2400, 64, 0, 1), (8192, 64, 0, 1), (16384, 64, 0, 1), (38896, 64, 0, 1)]
    for n_kv, nt, keep, lng in table:
        if n_kv < 32:
            continue
        for form in (0, 1):
            p = plan(A, 32, n_kv - 32, form=form)
            assert (p.family, p.R, p.nt, p.keep, p.long, p.lds, p.block, p.pitch) == (FLASH, 32, nt, keep, lng, FLASH_LDS[nt], 512, 32 * nt + 8), (n_kv, p)
            assert (p.packed, p.scratch, p.nt_total, p.ctx_tab, p.persistent, p.gx, p.gy, p.dbg) == (0, 0, 0, 1, 0, 2, 1, 0), (n_kv, p)
    assert plan(A, 31, 0).family == ROWS and plan(A, 32, 0).family == FLASH
    # FQ_ATTN_KEEP=0: K.Q twice at pitch 16 / 32; 33..64 tiles move to pitch 74
    for n_kv, nt in ((512, 16), (513, 32), (1024, 32), (1025, 74), (2048, 74), (2049, 74), (2368, 74)):
        p = plan(A, 32, n_kv - 32, keep=0)
        assert (p.family, p.nt, p.keep, p.long) == (FLASH, nt, 0, 0), (n_kv, p)
    p = plan(A, 32, 2369 - 32, keep=0)
    assert (p.family, p.nt, p.keep, p.long) == (FLASH, 64, 0, 1), p
    # FQ_ATTN_FLASH_LONG=0: the scratch form beyond 74 tiles (forms 0 and 1 alike), flash up to there
    for form in (0, 1):
        assert plan(A, 32, 2368 - 32, form=form, flash_long=0).family == FLASH
        p = plan(A, 33, 2400, form=form, flash_long=0)
        assert (p.family, p.R, p.gx, p.gy, p.block, p.lds, p.pitch, p.scratch) == (MFMA_SCRATCH, 32, 2, 2, 256, 0, 2464, 2 * 2 * 32 * 2464 * 4), p
    # FQ_ATTN_FLASH=0: form 0 is the scratch form at every length, form 1 still the flash form
    p = plan(A, 33, 5, flash=0)
    assert (p.family, p.gy, p.pitch, p.scratch) == (MFMA_SCRATCH, 2, 64, 2 * 2 * 32 * 64 * 4), p
    assert plan(A, 33, 5, flash=0, form=1).family == FLASH
    # form 32: the scratch form
    assert plan(A, 2048, 0, form=32, H=71).scratch == 64 * 71 * 32 * 2048 * 4
    # the other flash switches ride along
    assert plan(A, 32, 0, flash_tab=0).ctx_tab == 0 and plan(A, 32, 0, dbg=5).dbg == 5


def test_packed_keys(A):
    """from FQ_ATTN_PACK_MIN_N (256) tokens on the keys and values are re-laid first: 2 x 8192 bytes per KV head and key tile"""
    for N, n_past, HKV, packed in ((255, 0, 1, 0), (256, 0, 1, 1), (2048, 0, 1, 1), (512, 7680, 8, 1), (255, 3000, 8, 0)):
        p = plan(A, N, n_past, H=8 * HKV, HKV=HKV)
        tiles = (n_past + N + 31) // 32
        assert (p.family, p.packed, p.nt_total, p.scratch) == (FLASH, packed, tiles * packed, HKV * tiles * 16384 * packed), p
    assert plan(A, 64, 0, pack_min_n=64).packed == 1 and plan(A, 63, 0, pack_min_n=64).packed == 0 and plan(A, 2048, 0, pack_min_n=100000).packed == 0
    # no room for them: the same kernel on the cache as it lies
    p = plan(A, 512, 7680, cap=256 * 16384 - 1)
    assert (p.family, p.long, p.packed, p.nt_total, p.scratch) == (FLASH, 1, 0, 0, 0), p
    assert plan(A, 512, 7680, cap=256 * 16384).packed == 1


def test_persistent_workgroups(A):
    """one workgroup per CU taking (head, query tile) items from a counter once there are 4 items per CU"""
    for H, n_cu, first in ((71, 256, 449), (128, 256, 225), (71, 304, 545), (128, 64, 33)):        # H x ceil(N / 32) >= 4 n_cu
        p = plan(A, first - 1, 0, H=H, HKV=1, n_cu=n_cu)
        assert (p.family, p.persistent, p.gx, p.gy) == (FLASH, 0, H * ((first + 30) // 32), 1), (H, n_cu, p)
        p = plan(A, first, 0, H=H, HKV=1, n_cu=n_cu)
        assert (p.family, p.persistent, p.gx, p.gy) == (FLASH, 1, n_cu, 1), (H, n_cu, p)
        p = plan(A, first, 0, H=H, HKV=1, n_cu=n_cu, persist=0)
        assert (p.persistent, p.gx) == (0, H * ((first + 31) // 32)), (H, n_cu, p)


def test_forms_16_and_17(A):
    """the 16-token tiles: form 16 while (16 x (32 tiles + 4) + 1168) x 4 <= 158 KiB (2432 keys) and up to FQ_ATTN_MFMA16_MAXKV, form 17 while
    5632 + 16 x (32 tiles + 8) x 2 <= 158 KiB (4864 keys); beyond, the scratch form -- never the flash form"""
    for env in (dict(form=16), dict(mfma16=1)):
        p = plan(A, 64, 2432 - 64, H=3, **env)
        assert (p.family, p.R, p.gx, p.gy, p.block, p.lds, p.pitch, p.scratch) == (MFMA16, 16, 3, 4, 512, (16 * 2436 + 1168) * 4, 2436, 0), p
        assert plan(A, 64, 2433 - 64, **env).family == MFMA_SCRATCH
        p = plan(A, 33, 0, **env)
        assert (p.family, p.gy, p.lds, p.pitch) == (MFMA16, 3, (16 * 68 + 1168) * 4, 68), p
        assert plan(A, 64, 1000 - 64, mfma16_maxkv=1000, **env).family == MFMA16 and plan(A, 64, 1001 - 64, mfma16_maxkv=1000, **env).family == MFMA_SCRATCH
    for env in (dict(form=17), dict(mfma16h=1), dict(mfma16h=1, mfma16=1)):
        p = plan(A, 64, 4864 - 64, H=3, **env)
        assert (p.family, p.R, p.gx, p.gy, p.block, p.lds, p.pitch) == (MFMA16H, 16, 3, 4, 512, 5632 + 16 * 4872 * 2, 4872), p
        assert plan(A, 64, 4865 - 64, **env).family == MFMA_SCRATCH
        assert plan(A, 64, 1001 - 64, mfma16_maxkv=1000, **env).family == MFMA16H
    assert 5632 + 16 * 4872 * 2 <= 158 * KiB < 5632 + 16 * 4904 * 2 and (16 * 2436 + 1168) * 4 <= 158 * KiB < (16 * 2468 + 1168) * 4
    # a form that was set wins over the environment's
    assert plan(A, 64, 0, form=32, mfma16h=1).family == MFMA_SCRATCH and plan(A, 64, 0, form=1, mfma16=1).family == FLASH and plan(A, 64, 0, form=16, mfma16h=1).family == MFMA16
    assert plan(A, 31, 0, form=16).family == ROWS and plan(A, 31, 0, form=17).family == ROWS
    # beyond their limits without room for the scores: the rows forms
    p = plan(A, 64, 4865 - 64, form=17, cap=0)
    assert (p.family, p.R) == (ROWS, 2), p


def test_row_count_override(A):
    """FQ_ATTN_ROWS: 0 one token per workgroup; 8 / 4 / 2 where there are tokens enough and the rows fit 150 KiB, else the default count; set at all: neither the
    matrix pipe nor the scratch"""
    for N in (1, 3, 9, 512):
        p = plan(A, N, 100, rows=0)
        assert (p.family, p.R, p.gy) == (ONE, 1, N), p
    want = {8: [(1, 1), (2, 2), (3, 2), (4, 8), (9, 8), (512, 8)], 4: [(1, 1), (2, 2), (3, 2), (4, 4), (9, 4), (512, 4)], 2: [(1, 1), (2, 2), (3, 2), (4, 2), (9, 2), (512, 2)]}
    for force, rows in want.items():
        for N, R in rows:
            p = plan(A, N, 100, rows=force)
            assert (p.family, p.R, p.gy, p.lds, p.scratch) == (ROWS if R > 1 else ONE, R, (N + R - 1) // R, 8256 + R * row_bytes(100 + N), 0), (force, N, p)
    # 8 rows fit up to 4540 keys (8256 + 8 x 4 x 4540 = 153536), 4 up to 9084; beyond, the default count -- in LDS: no scratch form under the override
    assert (plan(A, 8, 4532, rows=8).R, plan(A, 8, 4533, rows=8).R) == (8, 2)
    assert (plan(A, 8, 3061, rows=4).R, plan(A, 8, 9076, rows=4).R, plan(A, 8, 9077, rows=4).R) == (4, 4, 2)
    for force in (8, 4, 2):
        p = plan(A, 8, 9077, rows=force)
        assert (p.family, p.R, p.lds) == (ROWS, 2, 8256 + 2 * row_bytes(9085)), p
    p = plan(A, 8, 18161, rows=2)
    assert (p.family, p.R) == (ONE, 1), p
    # any other value: the default count, still no matrix pipe and no scratch
    p = plan(A, 64, 0, rows=3)
    assert (p.family, p.R) == (ROWS, 4), p
    p = plan(A, 6, 3500, rows=3)
    assert (p.family, p.R) == (ROWS, 2), p


def test_matrix_pipe_and_scratch_off(A):
    p = plan(A, 40, 60, mfma=0)
    assert (p.family, p.R, p.gy, p.lds) == (ROWS, 4, 10, 8256 + 4 * 400), p
    p = plan(A, 512, 7680, mfma=0, H=71)
    assert (p.family, p.R, p.scratch) == (ROWS_SCRATCH, 4, 128 * 71 * 4 * 32768), p
    p = plan(A, 6, 3500, scratch=0)
    assert (p.family, p.R, p.gy, p.lds, p.scratch) == (ROWS, 2, 3, 8256 + 2 * 14032, 0), p
    p = plan(A, 512, 7680, scratch=0)       # (the flash form's packed keys are not what FQ_ATTN_SCRATCH is about)
    assert (p.family, p.packed) == (FLASH, 1), p
    p = plan(A, 512, 7680, scratch=0, f64=1)
    assert (p.family, p.R, p.scratch) == (ROWS, 2, 0), p


def test_scratch_cap_too_small(A):
    """the op-level cap (FQ_ATTN_SCRATCH_GB) or a context's own buffer: what does not fit is not asked for"""
    need = 2 * 2 * 4 * 14032
    assert plan(A, 6, 3500, cap=need).family == ROWS_SCRATCH
    p = plan(A, 6, 3500, cap=need - 1)
    assert (p.family, p.R, p.lds, p.scratch) == (ROWS, 2, 8256 + 2 * 14032, 0), p
    # the scratch form of the matrix pipe falls to the rows forms: four rows in LDS, four on the scratch where that fits, else two in LDS
    need = 2 * 2 * 32 * 64 * 4
    assert plan(A, 33, 5, form=32, cap=need).family == MFMA_SCRATCH
    p = plan(A, 33, 5, form=32, cap=need - 1)
    assert (p.family, p.R) == (ROWS, 4), p
    p = plan(A, 33, 5000, form=32, cap=2 * 2 * 32 * 5056 * 4 - 1)          # (a ragged batch: 9 four-row slices are smaller than 2 tiles of 32 rows)
    assert (p.family, p.R, p.gy, p.scratch) == (ROWS_SCRATCH, 4, 9, 9 * 2 * 4 * 4 * 5036), p
    big = 16 * 71 * 32 * 8192 * 4           # 512 tokens at 8192 keys, 71 heads: 1.19 GB of scores -- and as much in 4-row slices
    assert big == plan(A, 512, 7680, H=71, form=32).scratch == 128 * 71 * 4 * 32768
    p = plan(A, 512, 7680, H=71, form=32, scratch_gb=1)
    assert (p.family, p.R, p.scratch) == (ROWS, 2, 0), p
    p = plan(A, 2048, 14336, H=71, form=32)                    # 64 x 71 x 32 x 16384 x 4 = 9.5 GB and 4.8 GB: neither below 4 GiB
    assert (p.family, p.R, p.scratch) == (ROWS, 2, 0), p
    assert plan(A, 2048, 14336, H=71, form=32, scratch_gb=16).family == MFMA_SCRATCH


# ---- a context's scratch
def need_ref(n_batch, H, n_ctx, HKV, flash=True, cap=4 * GiB, pack_min_n=256):
    """fq_attention_scratch_need as it stood (with the LONG form on, k_attention_flash fits every n_ctx)"""
    if n_batch < 4:
        return 0
    tiles = (n_ctx + 31) // 32
    if n_batch >= 32 and flash:
        return HKV * tiles * 8192 * 2 if n_batch >= pack_min_n else 0
    ps = (n_ctx + 31) & ~31
    a = ((n_batch + 31) // 32) * H * 32 * ps * 4 if n_batch >= 32 else 0
    row = row_bytes(n_ctx)
    b = ((n_batch + 3) // 4) * H * 4 * row if 8256 + 4 * row > 56 * KiB else 0
    return min(max(a, b), cap)


NEED_GRID = [(nb, nc, H, HKV) for nb in (1, 3, 4, 8, 31, 32, 255, 256, 512, 2048) for nc in (32, 512, 2048, 3068, 3069, 8192, 16384) for H, HKV in ((71, 1), (128, 8), (2, 1))]


def test_context_scratch_need(A):
    for nb, nc, H, HKV in NEED_GRID:
        assert A.atf_scratch_need(nb, H, nc, HKV, sw_arr({})) == need_ref(nb, H, nc, HKV), (nb, nc, H, HKV)
        assert A.atf_scratch_need(nb, H, nc, HKV, sw_arr(dict(flash=0))) == need_ref(nb, H, nc, HKV, flash=False), (nb, nc, H, HKV)
        assert A.atf_scratch_need(nb, H, nc, HKV, sw_arr(dict(flash=0, scratch_gb=1))) == need_ref(nb, H, nc, HKV, flash=False, cap=GiB), (nb, nc, H, HKV)
        assert A.atf_scratch_need(nb, H, nc, HKV, sw_arr(dict(pack_min_n=32))) == need_ref(nb, H, nc, HKV, pack_min_n=32), (nb, nc, H, HKV)
    # FQ_ATTN_FLASH_LONG=0: beyond 74 tiles the scores of the scratch form
    assert A.atf_scratch_need(512, 71, 2368, 1, sw_arr(dict(flash_long=0))) == 74 * 16384
    assert A.atf_scratch_need(512, 71, 2369, 1, sw_arr(dict(flash_long=0))) == 16 * 71 * 32 * 2400 * 4
    # a few by hand
    assert A.atf_scratch_need(512, 71, 8192, 1, sw_arr({})) == 4 * MiB and A.atf_scratch_need(16, 71, 8192, 1, sw_arr({})) == 4 * 71 * 4 * 32768
    assert A.atf_scratch_need(16, 71, 2048, 1, sw_arr({})) == 0 and A.atf_scratch_need(2048, 71, 16384, 1, sw_arr(dict(flash=0))) == 4 * GiB


def test_context_scratch_gap_as_it_stands(A):
    """ADVICE.md's second finding, OPEN, recorded as it stands: a context of n_batch 512, n_ctx 8192 is sized for the packed keys alone (4 MiB), so the launches that
    want the 4-row scratch form there -- f64 order, a 16-token batch beyond ~3000 keys -- find the buffer too small and take 2 rows in LDS (36-40 against 32 ms per
    block at 8192 keys). The pull request that sizes the buffer for them changes these rows."""
    cap = A.atf_scratch_need(512, 71, 8192, 1, sw_arr({}))
    assert cap == 4 * MiB
    p = plan(A, 512, 7680, H=71, f64=1, cap=cap)
    assert (p.family, p.R, p.gy, p.lds, p.scratch) == (ROWS, 2, 256, 8256 + 2 * 32768, 0), p
    p = plan(A, 16, 3484, H=71, cap=cap)
    assert (p.family, p.R, p.gy, p.lds, p.scratch) == (ROWS, 2, 8, 8256 + 2 * 14000, 0), p
    # what they take with room (the op-level API's 4 GiB)
    assert plan(A, 512, 7680, H=71, f64=1).family == ROWS_SCRATCH and plan(A, 16, 3484, H=71).family == ROWS_SCRATCH
    # the default order's own launches of that context are served
    p = plan(A, 512, 7680, H=71, cap=cap)
    assert (p.family, p.long, p.packed, p.scratch) == (FLASH, 1, 1, cap), p


def test_a_context_never_grows_its_scratch(A):
    """every launch of a context -- any N <= n_batch, n_kv <= n_ctx, either order, either kind of pass -- planned against need(n_batch, n_ctx) asks for no more"""
    for nb, nc, H, HKV in NEED_GRID:
        for flash in (1, 0):
            cap = A.atf_scratch_need(nb, H, nc, HKV, sw_arr(dict(flash=flash)))
            for N in sorted({1, 2, 4, 5, 31, 32, 33, 255, 256, nb} & set(range(1, nb + 1))):
                for n_kv in sorted({N, 512, 2048, 2369, 3068, 3069, nc} & set(range(N, nc + 1))):
                    for kw in ({}, dict(f64=1), dict(form=32), dict(lockstep=1)):
                        p = plan(A, N, n_kv - N, H=H, HKV=HKV, cap=cap, flash=flash, **kw)
                        assert p.family > REFUSE_KEYS and p.scratch <= cap, (nb, nc, H, HKV, flash, N, n_kv, kw, p)
