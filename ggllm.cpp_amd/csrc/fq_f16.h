// fq_f16.h -- the F16 weight format: conversions and THE chain step of its mat-mul, shared by host and device code.
//
// The contract is the reference's scalar build of ggml_compute_forward_mul_mat_f16_f32 (ggml.c:11104-11316) over ggml_vec_dot_f16 (ggml.c:2306-2340):
//   1. the activation column is rounded element by element to fp16 (GGML_FP32_TO_FP16: to nearest even, subnormals kept);
//   2. sum is a DOUBLE that starts at 0; for i = 0 .. K-1 IN THAT ORDER  sum += (double)((float) w[i] * (float) x16[i]);
//   3. dst = (float) sum.
// The f32 product of two fp16 values is exact (11 x 11 significand bits, magnitudes 2^-48 .. 2^32), so fma(double w, double x, sum) is the same operation as
// the reference's multiply, widen, add: one rounding, of the same exact value. The ORDER is the contract: rows whose large terms cancel give other f32
// results in any other association (tests/test_f16_yardstick_cpu.py), so every form of the mat-mul walks a row through fq_f16_chain_step, element by element.
#pragma once
#include "fq_types.h"

FQ_HD uint16_t fq_f32_to_f16_bits(float f) {                                                              // round to nearest even, subnormals kept
#if defined(__HIP_DEVICE_COMPILE__)
    return fq_cvt_f16_bits(f);                        // never folded with the arithmetic that made f (fq_types.h)
#else
    return __builtin_bit_cast(uint16_t, (_Float16) f);
#endif
}
FQ_HD float    fq_f16_bits_to_f32(uint16_t h) { return (float) __builtin_bit_cast(_Float16, h); }         // exact
FQ_HD double   fq_f16_bits_to_f64(uint16_t h) { return (double) __builtin_bit_cast(_Float16, h); }        // exact

// one element of a row: sum + w * x with ONE rounding (the product is exact in f32 and in f64 alike)
FQ_HD double fq_f16_chain_step(double sum, double w, double x) { return __builtin_fma(w, x, sum); }

// row length the F16 kernels take (a 16-byte load is 8 weights; 32 keeps every tile edge on such a load: 4544 = 142 x 32)
#define FQ_F16_K_MULTIPLE 32
// the activation image of F16 weights: one column = K fp16 values, 16-byte aligned
FQ_HD size_t fq_f16_col_bytes(int64_t K) { return ((size_t) K * 2 + 15) & ~(size_t) 15; }
