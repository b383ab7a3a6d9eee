"""The launch key of a mat-mul (csrc/fq_mm_forms.h fq_mm_launch_key) on the CPU: tests/host/mm_forms_harness.cpp host-compiled with g++, default switches.
tests/test_mm_coverage_cpu.py takes its census from here; the GPU cases of tests/mm_shapes.py compare the device's own plan (ggml_hip_debug_mul_mat_plan)
with key(..) at 256 CUs."""
import ctypes as C
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CU = 256               # MI355X
KEY_LEN = 8
F16, REF, KQREF, GEMV, STREAM, TILE = range(6)
SK_RES, SK_KSHARE, SK_PLAIN, SK_KQ = 1, 2, 3, 4
_lib, _dir = None, None


def harness():
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.TemporaryDirectory(prefix="mmk")
        out = os.path.join(_dir.name, "libmm_forms_host.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I", os.path.join(ROOT, "ggllm.cpp_amd", "csrc"),
                               "-o", out, os.path.join(ROOT, "tests", "host", "mm_forms_harness.cpp")])
        _lib = C.CDLL(out)
        ll, i = C.c_longlong, C.c_int
        _lib.mmf_launch_key.restype, _lib.mmf_launch_key.argtypes = None, [i, ll, ll, ll, i, i, i, i, i, i, C.POINTER(i)]
    return _lib


def mode_args(mode):
    """(ref_order, sequential, forced cfg) of a mode of tests/mm_shapes.py"""
    if mode == "default":
        return 0, 0, -1
    if mode == "seq":
        return 0, 1, -1
    if mode in ("ref1", "ref2"):
        return int(mode[3]), 1, -1
    assert mode.startswith("cfg"), mode
    return 0, 0, int(mode[3:])


def key(t, K, M, N, mode="default", from3=0, n_cu=N_CU):
    """(type, family, S, more than one pass, stream kind, four facts of the form)"""
    ref, seq, cfg = mode_args(mode)
    o = (C.c_int * KEY_LEN)()
    harness().mmf_launch_key(t, M, K, N, n_cu, ref, seq, 0, cfg, from3, o)
    return (t,) + tuple(o)
