// Element-wise host side of the scalar-arithmetic sweep (tests/scalar_domains.py, tests/test_scalar_domains_cpu.py, tests/test_gpu_scalar_arith.py):
//   scalar_libm_eval  the REFERENCE of the libm group: the host libm's expf, logf, log2f, powf and x86's cvttss2si, element by element;
//   scalar_host_eval  the g++ build of the FQ_HD routines themselves (the host branch of those that have a device branch), so that a mismatch on the
//                     device can be told from a host libm this restatement does not match, or from a domain that is wrong.
// fn is the enum of include/ggml-hip-ops.h (GGML_HIP_SCALAR_*); a, b and out are raw bits, as ggml_hip_debug_scalar_eval takes them. Built with -fwrapv:
// the accumulator cases of fq_dot4 / fq_dot2 wrap on purpose. (sample_chain_harness.cpp is included for chain_powf_pair, the random-pair generator the
// exhaustive host test uses, so that both see the same pairs.)
#include "sample_chain_harness.cpp"
#include "fq_wquant.h"
#include "fq_kdot.h"
#include "../../include/ggml-hip-ops.h"
#include <xmmintrin.h>

template <class F>
static void each(int64_t n, int n_threads, F f) {
    std::vector<std::thread> th;
    for (int t = 0; t < n_threads; ++t)
        th.emplace_back([=] { for (int64_t i = n / n_threads * t, e = t + 1 == n_threads ? n : n / n_threads * (t + 1); i < e; ++i) f(i); });
    for (auto & x : th) x.join();
}

extern "C" {

// 0, or 1 for an fn the host libm / x86 has no word on
int scalar_libm_eval(int fn, const uint32_t * a, const uint32_t * b, int64_t n, uint32_t * out, int n_threads) {
    switch (fn) {
        case GGML_HIP_SCALAR_EXPF:  each(n, n_threads, [=](int64_t i) { out[i] = fq_f2u(expf(fq_u2f(a[i]))); }); return 0;
        case GGML_HIP_SCALAR_LOGF:  each(n, n_threads, [=](int64_t i) { out[i] = fq_f2u(logf(fq_u2f(a[i]))); }); return 0;
        case GGML_HIP_SCALAR_LOG2F: each(n, n_threads, [=](int64_t i) { out[i] = fq_f2u(log2f(fq_u2f(a[i]))); }); return 0;
        case GGML_HIP_SCALAR_POWF:  each(n, n_threads, [=](int64_t i) { out[i] = fq_f2u(powf(fq_u2f(a[i]), fq_u2f(b[i]))); }); return 0;
        case GGML_HIP_SCALAR_F2I_X86: each(n, n_threads, [=](int64_t i) { out[i] = (uint32_t) _mm_cvttss_si32(_mm_set_ss(fq_u2f(a[i]))); }); return 0;
        default: return 1;
    }
}

// 0, or 1 for an fn whose routine has no g++ build (f2h_bits / h2f_bits are device functions, fq_f16.h's casts need _Float16)
int scalar_host_eval(int fn, const uint32_t * a, const uint32_t * b, int64_t n, uint32_t * out, int n_threads) {
#define EACH(EXPR) each(n, n_threads, [=](int64_t i) { out[i] = (uint32_t)(EXPR); }); return 0
    switch (fn) {
        case GGML_HIP_SCALAR_EXPF:  EACH(fq_f2u(fq_expf(fq_u2f(a[i]))));
        case GGML_HIP_SCALAR_LOGF:  EACH(fq_f2u(fq_logf(fq_u2f(a[i]))));
        case GGML_HIP_SCALAR_LOG2F: EACH(fq_f2u(fq_log2f(fq_u2f(a[i]))));
        case GGML_HIP_SCALAR_POWF:  EACH(fq_f2u(fq_powf(fq_u2f(a[i]), fq_u2f(b[i]))));
        case GGML_HIP_SCALAR_F2I_X86: EACH(fq_f2i_x86(fq_u2f(a[i])));
        case GGML_HIP_SCALAR_NEGLIGIBLE_F: EACH(fq_negligible_f(fq_u2f(a[i]), fq_u2f(b[i])) ? 1 : 0);
        case GGML_HIP_SCALAR_NEGLIGIBLE_D: EACH(fq_negligible_d((double) fq_u2f(a[i]), (double) fq_u2f(b[i])) ? 1 : 0);
        case GGML_HIP_SCALAR_F2H:         EACH(fq_f2h(fq_u2f(a[i])));
        case GGML_HIP_SCALAR_F2H_PRODUCT: EACH(fq_f2h(fq_u2f(a[i]) * fq_u2f(b[i])));
        case GGML_HIP_SCALAR_H2F:         EACH(fq_f2u(fq_h2f((uint16_t) a[i])));
        case GGML_HIP_SCALAR_DOT4:        EACH(fq_dot4(a[i], b[i], 0));
        case GGML_HIP_SCALAR_DOT4_C_HIGH: EACH(fq_dot4(a[i], b[i], 0x7FFFFF00));
        case GGML_HIP_SCALAR_DOT4_C_LOW:  EACH(fq_dot4(a[i], b[i], -0x7FFFFF00));
        case GGML_HIP_SCALAR_DOT4_C_MID:  EACH(fq_dot4(a[i], b[i], 12345));
        case GGML_HIP_SCALAR_DOT4Z:       EACH(fq_dot4z(a[i], b[i]));
        case GGML_HIP_SCALAR_DOT2:        EACH(fq_dot2(a[i], b[i], 0));
        case GGML_HIP_SCALAR_DOT2_C_HIGH: EACH(fq_dot2(a[i], b[i], 0x7FFFFF00));
        case GGML_HIP_SCALAR_DOT2_C_LOW:  EACH(fq_dot2(a[i], b[i], -0x7FFFFF00));
        case GGML_HIP_SCALAR_DOT2_C_MID:  EACH(fq_dot2(a[i], b[i], 12345));
        case GGML_HIP_SCALAR_DOT2Z:       EACH(fq_dot2z(a[i], b[i]));
        case GGML_HIP_SCALAR_PACK16:      EACH(fq_pack16((int) a[i], (int) b[i]));
        case GGML_HIP_SCALAR_PK_SUB16:    EACH(fq_pk_sub16(a[i], b[i]));
        case GGML_HIP_SCALAR_MUL24:       EACH(fq_mul24((int) a[i], (int) b[i]));
        default: return 1;
    }
#undef EACH
}

// pairs [first, first + n) of chain_powf_pair's sweep
void scalar_powf_pairs(uint64_t seed, uint64_t first, int64_t n, uint32_t * x, uint32_t * y) {
    for (int64_t i = 0; i < n; ++i) {
        float fx, fy;
        chain_powf_pair(seed, first + (uint64_t) i, &fx, &fy);
        x[i] = fq_f2u(fx); y[i] = fq_f2u(fy);
    }
}

}
