// kernels_scalar_check.hip -- the FQ_HD scalar routines as hipcc compiles them for the device, one routine per launch, one element per lane: what the
// host tests establish for the g++ build of the same headers (exactness against the host libm, the fp16 conversions, the integer units) is checked here for
// the code the sampler, scorer, quantizer and k-quant kernels actually run (tests/test_gpu_scalar_arith.py compares every element with an independent
// reference). Every case calls the production routine from the production header; nothing is restated, and there is no inline assembly of this file's own.
// Built with -fno-slp-vectorize like kernels_sample.hip, whose routines most of these are.
#include "fq_device.h"          // f2h_bits, h2f_bits
#include "hip_context.h"
#include "fq_sample_chain.h"    // fq_expf, fq_negligible_* (fq_sample.h), fq_logf, fq_log2f, fq_powf, fq_f2i_x86
#include "fq_wquant.h"          // fq_f2h
#include "fq_f16.h"             // fq_f32_to_f16_bits, fq_f16_bits_to_f32
#include "fq_kdot.h"            // fq_dot2, fq_dot2z, fq_pack16, fq_pk_sub16, fq_mul24 (fq_units.h: fq_dot4, fq_dot4z, fq_h2f)
#include "../../include/ggml-hip-ops.h"

#define FQ_SCK_THREADS 256

template <int FN> struct sck_two_args { static constexpr bool value = FN == GGML_HIP_SCALAR_POWF || FN == GGML_HIP_SCALAR_NEGLIGIBLE_F || FN == GGML_HIP_SCALAR_NEGLIGIBLE_D ||
    (FN >= GGML_HIP_SCALAR_F2H_BITS_PRODUCT && FN <= GGML_HIP_SCALAR_F32_TO_F16_BITS_PRODUCT) || FN >= GGML_HIP_SCALAR_DOT4; };

template <int FN>
__device__ __forceinline__ uint32_t sck_eval(uint32_t a, uint32_t b) {
    const float x = fq_u2f(a), y = fq_u2f(b);
    if constexpr (FN == GGML_HIP_SCALAR_EXPF)  return fq_f2u(fq_expf(x));
    if constexpr (FN == GGML_HIP_SCALAR_LOGF)  return fq_f2u(fq_logf(x));
    if constexpr (FN == GGML_HIP_SCALAR_LOG2F) return fq_f2u(fq_log2f(x));
    if constexpr (FN == GGML_HIP_SCALAR_POWF)  return fq_f2u(fq_powf(x, y));
    if constexpr (FN == GGML_HIP_SCALAR_F2I_X86) return (uint32_t) fq_f2i_x86(x);
    if constexpr (FN == GGML_HIP_SCALAR_NEGLIGIBLE_F) return fq_negligible_f(x, y) ? 1u : 0u;
    if constexpr (FN == GGML_HIP_SCALAR_NEGLIGIBLE_D) return fq_negligible_d((double) x, (double) y) ? 1u : 0u;
    if constexpr (FN == GGML_HIP_SCALAR_F2H_BITS)        return f2h_bits(x);
    if constexpr (FN == GGML_HIP_SCALAR_F2H)             return fq_f2h(x);
    if constexpr (FN == GGML_HIP_SCALAR_F32_TO_F16_BITS) return fq_f32_to_f16_bits(x);
    if constexpr (FN == GGML_HIP_SCALAR_F2H_BITS_PRODUCT)        return f2h_bits(x * y);
    if constexpr (FN == GGML_HIP_SCALAR_F2H_PRODUCT)             return fq_f2h(x * y);
    if constexpr (FN == GGML_HIP_SCALAR_F32_TO_F16_BITS_PRODUCT) return fq_f32_to_f16_bits(x * y);
    if constexpr (FN == GGML_HIP_SCALAR_H2F_BITS)        return fq_f2u(h2f_bits((uint16_t) a));
    if constexpr (FN == GGML_HIP_SCALAR_H2F)             return fq_f2u(fq_h2f((uint16_t) a));
    if constexpr (FN == GGML_HIP_SCALAR_F16_BITS_TO_F32) return fq_f2u(fq_f16_bits_to_f32((uint16_t) a));
    if constexpr (FN == GGML_HIP_SCALAR_DOT4)        return (uint32_t) fq_dot4(a, b, 0);
    if constexpr (FN == GGML_HIP_SCALAR_DOT4_C_HIGH) return (uint32_t) fq_dot4(a, b, 0x7FFFFF00);
    if constexpr (FN == GGML_HIP_SCALAR_DOT4_C_LOW)  return (uint32_t) fq_dot4(a, b, -0x7FFFFF00);
    if constexpr (FN == GGML_HIP_SCALAR_DOT4_C_MID)  return (uint32_t) fq_dot4(a, b, 12345);
    if constexpr (FN == GGML_HIP_SCALAR_DOT4Z)       return (uint32_t) fq_dot4z(a, b);
    if constexpr (FN == GGML_HIP_SCALAR_DOT2)        return (uint32_t) fq_dot2(a, b, 0);
    if constexpr (FN == GGML_HIP_SCALAR_DOT2_C_HIGH) return (uint32_t) fq_dot2(a, b, 0x7FFFFF00);
    if constexpr (FN == GGML_HIP_SCALAR_DOT2_C_LOW)  return (uint32_t) fq_dot2(a, b, -0x7FFFFF00);
    if constexpr (FN == GGML_HIP_SCALAR_DOT2_C_MID)  return (uint32_t) fq_dot2(a, b, 12345);
    if constexpr (FN == GGML_HIP_SCALAR_DOT2Z)       return (uint32_t) fq_dot2z(a, b);
    if constexpr (FN == GGML_HIP_SCALAR_PACK16)      return fq_pack16((int) a, (int) b);
    if constexpr (FN == GGML_HIP_SCALAR_PK_SUB16)    return fq_pk_sub16(a, b);
    if constexpr (FN == GGML_HIP_SCALAR_MUL24)       return (uint32_t) fq_mul24((int) a, (int) b);
    return 0u;
}

// one lane per element, grid-stride, bounded by n; b is read only by the two-argument routines
template <int FN>
__global__ void __launch_bounds__(FQ_SCK_THREADS) k_scalar_eval(const uint32_t * __restrict__ a, const uint32_t * __restrict__ b, int64_t n, uint32_t * __restrict__ out) {
    const int64_t step = (int64_t) gridDim.x * FQ_SCK_THREADS;
    for (int64_t i = (int64_t) blockIdx.x * FQ_SCK_THREADS + threadIdx.x; i < n; i += step) {
        uint32_t bi = 0u;
        if constexpr (sck_two_args<FN>::value) bi = b[i];
        out[i] = sck_eval<FN>(a[i], bi);
    }
}

template <int FN>
static int sck_launch(const uint32_t * a, const uint32_t * b, int64_t n, uint32_t * out, hipStream_t st) {
    if (sck_two_args<FN>::value && !b) return 1;
    const int64_t blocks = (n + FQ_SCK_THREADS - 1) / FQ_SCK_THREADS;
    hipLaunchKernelGGL(k_scalar_eval<FN>, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(FQ_SCK_THREADS), 0, st, a, b, n, out);
    return 0;
}

// ------------------------------------------------------------------------------------------------ C ABI (include/ggml-hip-ops.h)
extern "C" int ggml_hip_debug_scalar_eval(int fn, const uint32_t * a_dev, const uint32_t * b_dev, int64_t n, uint32_t * out_dev) {
    if (!a_dev || !out_dev || n < 0) return 1;
    if (n == 0) return fn >= 0 && fn < GGML_HIP_SCALAR_COUNT ? 0 : 1;
    hipStream_t st = fq_ctx().stream;
    switch (fn) {
#define SCK_CASE(F) case F: return sck_launch<F>(a_dev, b_dev, n, out_dev, st);
        SCK_CASE(GGML_HIP_SCALAR_EXPF) SCK_CASE(GGML_HIP_SCALAR_LOGF) SCK_CASE(GGML_HIP_SCALAR_LOG2F) SCK_CASE(GGML_HIP_SCALAR_POWF) SCK_CASE(GGML_HIP_SCALAR_F2I_X86)
        SCK_CASE(GGML_HIP_SCALAR_NEGLIGIBLE_F) SCK_CASE(GGML_HIP_SCALAR_NEGLIGIBLE_D)
        SCK_CASE(GGML_HIP_SCALAR_F2H_BITS) SCK_CASE(GGML_HIP_SCALAR_F2H) SCK_CASE(GGML_HIP_SCALAR_F32_TO_F16_BITS)
        SCK_CASE(GGML_HIP_SCALAR_H2F_BITS) SCK_CASE(GGML_HIP_SCALAR_H2F) SCK_CASE(GGML_HIP_SCALAR_F16_BITS_TO_F32)
        SCK_CASE(GGML_HIP_SCALAR_F2H_BITS_PRODUCT) SCK_CASE(GGML_HIP_SCALAR_F2H_PRODUCT) SCK_CASE(GGML_HIP_SCALAR_F32_TO_F16_BITS_PRODUCT)
        SCK_CASE(GGML_HIP_SCALAR_DOT4) SCK_CASE(GGML_HIP_SCALAR_DOT4_C_HIGH) SCK_CASE(GGML_HIP_SCALAR_DOT4_C_LOW) SCK_CASE(GGML_HIP_SCALAR_DOT4_C_MID) SCK_CASE(GGML_HIP_SCALAR_DOT4Z)
        SCK_CASE(GGML_HIP_SCALAR_DOT2) SCK_CASE(GGML_HIP_SCALAR_DOT2_C_HIGH) SCK_CASE(GGML_HIP_SCALAR_DOT2_C_LOW) SCK_CASE(GGML_HIP_SCALAR_DOT2_C_MID) SCK_CASE(GGML_HIP_SCALAR_DOT2Z)
        SCK_CASE(GGML_HIP_SCALAR_PACK16) SCK_CASE(GGML_HIP_SCALAR_PK_SUB16) SCK_CASE(GGML_HIP_SCALAR_MUL24)
#undef SCK_CASE
        default: return 1;
    }
}
