"""GPU: every attention kernel's soft-max over the whole fp16 range of the EXP table -- the prefill forms on the matrix pipe (scratch, flash at every pitch and
LONG, 16-token tiles), the short routes (k_attention, 2 and 4 rows per workgroup, score rows in the global scratch) and the decode op, in both orders --
bit for bit against the numpy soft_max of tests/softmax_edges.py (which test_softmax_edges_cpu.py ties to the oracle): every index 0x8000 .. 0xFC00, the
formula's fix-list inputs and thresholds, subnormal results, differences where one rounding and two part, uniform and saturated rows, masked keys that hold
the largest score. The same launches run again in child processes with the in-kernel formula in place of the table gather (the switches are read once)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ggllm_cpp_amd as g
import softmax_edges as se

pytestmark = pytest.mark.gpu

CHECKS = se.gpu_checks()
GROUPS = sorted({c[0] for c in CHECKS})
FORMULA_ENVS = [{"GGML_HIP_EXP_FORMULA": "1", "FQ_ATTN_FLASH_TAB": "0"},
                {"GGML_HIP_EXP_FORMULA": "1", "FQ_ATTN_FLASH_TAB": "0", "FQ_ATTN_KEEP": "0", "FQ_ATTN_PERSIST": "0"}]


@pytest.fixture(scope="module")
def G():
    return se.Gpu()


def test_device_fix_list_is_the_headers(G):
    """the inputs the formula's fast path leaves undecided on this device, with the table's entries, are csrc/fq_exp_fix.h's: the families aim at the same inputs
    on the CPU and here"""
    assert G.fix == se.fix_list_from_header()


@pytest.mark.parametrize("check", CHECKS, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in CHECKS])
def test_soft_max_edges(G, check):
    bad = [b for b in check[3](G) if b]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("env", FORMULA_ENVS, ids=["formula", "formula-twice-nopersist"])
def test_soft_max_edges_with_the_formula_in_the_kernels(env, group):
    """GGML_HIP_EXP_FORMULA=1 FQ_ATTN_FLASH_TAB=0 (and the flash form's K.Q-twice, one-workgroup-per-item code): every attention kernel computes the entries
    with its own inlined exp_f16_formula; the child asserts the formula is in use, runs the group's launches and prints one line per (route, family)"""
    r = subprocess.run([sys.executable, os.path.abspath(se.__file__), group], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith(group + " ")]
    assert len(lines) == sum(c[0] == group for c in CHECKS) and all(l.endswith(": ok") for l in lines), r.stdout


def test_gelu_index_conversion_at_the_ties(G, oracle):
    """ggml_hip_gelu's f32 -> fp16 index conversion (the soft-max's own) at family R's ties and near-ties of either sign, at +-65504 / +-65520 / +-1e5 and at the
    fp16-subnormal magnitudes: the oracle's GELU, bit for bit"""
    m, _, _ = se.r_rows()
    ulp = np.spacing(m)
    sub = np.arange(1, 0x0400, dtype=np.uint16).view(np.float16).astype(np.float32)
    x = np.concatenate([m, m - ulp, m + ulp, sub, sub + np.float32(2.0 ** -26), np.float32([65504.0, 65519.9, 65520.0, 1.0e5, 0.0])]).astype(np.float32)
    x = np.concatenate([x, -x])
    L = G.L
    xb, yb = g.DevBuf(host=x), g.DevBuf(x.nbytes)
    try:
        L.ggml_hip_memset(yb.ptr, 0xFF, x.nbytes)
        L.ggml_hip_gelu(xb.ptr, yb.ptr, x.size)
        got = yb.to_host(np.float32, x.shape)
    finally:
        xb.free()
        yb.free()
    exp = oracle.gelu(x)
    nan = np.isnan(exp)                                     # (gelu(-inf) = -inf x 0: the payload is the host libm's)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), exp[~nan].view(np.uint32))
