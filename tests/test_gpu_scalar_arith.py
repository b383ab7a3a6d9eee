"""GPU: the shared host / device scalar routines -- the libm restatements the sampler and the scorer call per element, the fp16 conversions of the
epilogues and quantizers, the integer units of the k-quant dots -- as hipcc compiles them for gfx950, element by element against an independent reference
(tests/scalar_domains.py: the host libm, numpy's conversions, numpy integer arithmetic) on the domains tests/test_scalar_domains_cpu.py holds the g++
build of the same headers to. One test per routine; every element is compared as bits, and only two NaN results count as equal.

The host tests establish the restatements' exactness for x86 object code; the kernels run what ggml_hip_debug_scalar_eval runs here
(csrc/kernels_scalar_check.hip calls each routine from its production header), including the branches under __HIP_DEVICE_COMPILE__ and whatever the
kernel descriptor's float modes make of subnormal inputs and results."""
import numpy as np
import pytest

import ggllm_cpp_amd as g
import scalar_domains as sd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    g.init(0)
    return sd.build_harness(tmp_path_factory.mktemp("scalar"))


def _run(name, parts, H):
    """every part through the device; returns (a, b, device, reference) of the mismatching elements, all parts together"""
    total, out = 0, [np.zeros(0, np.uint32)] * 4
    for label, a, b in parts:
        want = sd.reference(name, a, b, H)
        if name in sd.LIBM:
            host = sd.host_eval(H, name, a, b)
            bad = sd.mismatches(name, host, want)
            assert bad.size == 0, "the HOST build of fq_%s disagrees with this machine's libm (not a device finding): %s" % (name, sd.report(label, a, b, host, want, bad, "host build"))
        got = g.scalar_eval(name, a, b)
        bad = sd.mismatches(name, got, want)
        total += a.size
        print("%s: %d elements, %d mismatches" % (label, a.size, bad.size))
        out = [np.concatenate([o, (np.zeros(a.size, np.uint32) if v is None else v)[bad]]) for o, v in zip(out, (a, b, got, want))]
    print("%s: %d elements in all, %d mismatches" % (name, total, out[0].size))
    return total, out


def _assert_none(name, total, bad):
    a, b, got, want = bad
    assert a.size == 0, sd.report(name, a, b, got, want, np.arange(a.size))


@pytest.mark.parametrize("name", [n for n in sd.ALL if n != "powf"])
def test_device_build_equals_reference(H, name):
    """(the *_product cases: the conversion of a product written in the call. A plain (_Float16)(a * b) is selected as v_fma_mixlo_f16 a, b, 0, which rounds
    the exact product once and turns a -0 product into +0: 61 470 of 30 478 763 elements differed from the reference for f2h_bits and fq_f32_to_f16_bits
    -- 61 460 signed zeros and 10 roundings such as 0x477feffe * 0x3f800001 = 65504 instead of inf -- until all three routines converted explicitly,
    csrc/fq_types.h fq_cvt_f16_bits. Zero is asserted for all three.)"""
    _assert_none(name, *_run(name, sd.domain(name, H), H))


@pytest.mark.parametrize("piece", sd.POWF_PIECES)
def test_device_powf_equals_libm(H, piece):
    _assert_none("powf " + piece, *_run("powf", sd.powf_domain(H, (piece,)), H))


def test_entry_refuses_what_it_cannot_run(H):
    L = g.load()
    buf = g.DevBuf(host=np.zeros(64, np.uint32))
    try:
        assert L.ggml_hip_debug_scalar_eval(len(sd.FN), buf.ptr, buf.ptr, 64, buf.ptr) == 1 and L.ggml_hip_debug_scalar_eval(-1, buf.ptr, buf.ptr, 64, buf.ptr) == 1
        assert L.ggml_hip_debug_scalar_eval(sd.FN["expf"], None, None, 64, buf.ptr) == 1 and L.ggml_hip_debug_scalar_eval(sd.FN["expf"], buf.ptr, None, 64, None) == 1
        assert L.ggml_hip_debug_scalar_eval(sd.FN["powf"], buf.ptr, None, 64, buf.ptr) == 1            # a two-argument routine needs b
        assert L.ggml_hip_debug_scalar_eval(sd.FN["expf"], buf.ptr, None, 64, buf.ptr) == 0            # a one-argument routine does not
        assert (buf.to_host(np.uint32, (64,)) == 0x3F800000).all()
    finally:
        buf.free()
