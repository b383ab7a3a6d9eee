// fq_sample.h -- falcon_main's default sampler chain (examples/falcon/falcon_main.cpp:896-980, libfalcon.cpp:3038-3466),
// restated once for the device sampler (kernels_sample.hip) and a host test (tests/test_sample_cpu.py compiles this header
// with g++ and checks it against the reference's own functions).
//
// What must be reproduced bit for bit:
//   * the host libm's expf (glibc's e_expf.c in the FMA variant its ifunc selects on an FMA-capable host: five fused
//     multiply-adds in double, one rounding to float at the end) -- fq_expf;
//   * std::mt19937 (seed, twist, tempering), std::generate_canonical<double, 53> and libstdc++'s discrete_distribution
//     (bits/random.tcc: no draw for fewer than two weights, double sum, normalised partial sums, last entry forced to 1,
//     lower_bound of the uniform draw) -- fq_mt_*, fq_canonical, fq_sample_tail;
//   * the f32 sums of the softmaxes (sequential, in sorted order).
// The sums run over candidates sorted by value, descending: a term below half an ulp of the running sum cannot change it,
// and neither can any later (smaller) term, so the scans stop there -- exact, not an approximation. No contraction: every
// fused operation is an explicit fma (the Makefile passes -ffp-contract=off).
#pragma once
#include "fq_types.h"
#include <math.h>
#include <stdint.h>

#define FQ_MT_N 624
#define FQ_MT_M 397
#define FQ_SAMPLE_MAX_BIAS 16

FQ_HD uint32_t fq_f2u(float x) { uint32_t u; __builtin_memcpy(&u, &x, 4); return u; }
FQ_HD float fq_u2f(uint32_t u) { float x; __builtin_memcpy(&x, &u, 4); return x; }
FQ_HD uint64_t fq_d2u(double x) { uint64_t u; __builtin_memcpy(&u, &x, 8); return u; }
FQ_HD double fq_u2d(uint64_t u) { double x; __builtin_memcpy(&x, &u, 8); return x; }

// glibc expf (sysdeps/ieee754/flt-32/e_expf.c, EXP2F_TABLE_BITS 5), multiply-adds fused as in its FMA build
FQ_HD float fq_expf(float x) {
    const uint64_t T[32] = {
        0x3ff0000000000000ull, 0x3fefd9b0d3158574ull, 0x3fefb5586cf9890full, 0x3fef9301d0125b51ull, 0x3fef72b83c7d517bull, 0x3fef54873168b9aaull,
        0x3fef387a6e756238ull, 0x3fef1e9df51fdee1ull, 0x3fef06fe0a31b715ull, 0x3feef1a7373aa9cbull, 0x3feedea64c123422ull, 0x3feece086061892dull,
        0x3feebfdad5362a27ull, 0x3feeb42b569d4f82ull, 0x3feeab07dd485429ull, 0x3feea47eb03a5585ull, 0x3feea09e667f3bcdull, 0x3fee9f75e8ec5f74ull,
        0x3feea11473eb0187ull, 0x3feea589994cce13ull, 0x3feeace5422aa0dbull, 0x3feeb737b0cdc5e5ull, 0x3feec49182a3f090ull, 0x3feed503b23e255dull,
        0x3feee89f995ad3adull, 0x3feeff76f2fb5e47ull, 0x3fef199bdd85529cull, 0x3fef3720dcef9069ull, 0x3fef5818dcfba487ull, 0x3fef7c97337b9b5full,
        0x3fefa4afa2a490daull, 0x3fefd0765b6e4540ull };
    const double InvLn2N = 0x1.71547652b82fep+5, SHIFT = 0x1.8p+52;
    const double C0 = 0x1.c6af84b912394p-20, C1 = 0x1.ebfce50fac4f3p-13, C2 = 0x1.62e42ff0c52d6p-6;     // poly / N^3, N^2, N
    const uint32_t abstop = (fq_f2u(x) >> 20) & 0x7ff;
    if (abstop >= ((fq_f2u(88.0f) >> 20) & 0x7ff)) {
        if (fq_f2u(x) == fq_f2u(-INFINITY)) return 0.0f;
        if (abstop >= ((fq_f2u(INFINITY) >> 20) & 0x7ff)) return x + x;
        if (x > 0x1.62e42ep6f) return INFINITY;
        if (x < -0x1.9fe368p6f) return 0.0f;
    }
    const double xd = (double) x;
    double kd = fma(InvLn2N, xd, SHIFT);
    const uint64_t ki = fq_d2u(kd);
    kd -= SHIFT;
    const double r = fma(InvLn2N, xd, -kd);
    const uint64_t t = T[ki % 32] + (ki << 47);
    const double s = fq_u2d(t);
    const double z = fma(C0, r, C1);
    const double r2 = r * r;
    double y = fma(C2, r, 1.0);
    y = fma(z, r2, y);
    y = y * s;
    return (float) y;
}

// ---- std::mt19937 (libstdc++ bits/random.tcc): state mt[0..624), index *mti
FQ_HD void fq_mt_seed(uint32_t * mt, int * mti, uint32_t seed) {
    mt[0] = seed;
    for (int i = 1; i < FQ_MT_N; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t) i;
    *mti = FQ_MT_N;
}
FQ_HD void fq_mt_twist(uint32_t * mt) {
    const uint32_t UP = 0x80000000u, LO = 0x7fffffffu, A = 0x9908b0dfu;
    for (int k = 0; k < FQ_MT_N - FQ_MT_M; ++k) {
        const uint32_t y = (mt[k] & UP) | (mt[k + 1] & LO);
        mt[k] = mt[k + FQ_MT_M] ^ (y >> 1) ^ ((y & 1u) ? A : 0u);
    }
    for (int k = FQ_MT_N - FQ_MT_M; k < FQ_MT_N - 1; ++k) {
        const uint32_t y = (mt[k] & UP) | (mt[k + 1] & LO);
        mt[k] = mt[k + (FQ_MT_M - FQ_MT_N)] ^ (y >> 1) ^ ((y & 1u) ? A : 0u);
    }
    const uint32_t y = (mt[FQ_MT_N - 1] & UP) | (mt[0] & LO);
    mt[FQ_MT_N - 1] = mt[FQ_MT_M - 1] ^ (y >> 1) ^ ((y & 1u) ? A : 0u);
}
FQ_HD uint32_t fq_mt_next(uint32_t * mt, int * mti) {
    if (*mti >= FQ_MT_N) { fq_mt_twist(mt); *mti = 0; }
    uint32_t y = mt[(*mti)++];
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}
// std::generate_canonical<double, 53>(mt19937): two draws, s = g1 + g2 * 2^32, s / 2^64, clamped below 1
FQ_HD double fq_canonical(uint32_t * mt, int * mti) {
    double s = (double) fq_mt_next(mt, mti);
    s += (double) fq_mt_next(mt, mti) * 4294967296.0;
    double u = s / 18446744073709551616.0;
    if (u >= 1.0) u = 0x1.fffffffffffffp-1;      // nextafter(1, 0)
    return u;
}

// sum + t == sum for this term (and, the terms being non-increasing, for every later one)
FQ_HD bool fq_negligible_f(float t, float sum) { return 2.0f * t < nextafterf(sum, INFINITY) - sum; }
FQ_HD bool fq_negligible_d(double t, double sum) { return 2.0 * t < nextafter(sum, (double) INFINITY) - sum; }

// ---- per-candidate logit edits in falcon_main's order: logit bias (bias_on: the id has an entry), repetition penalty and
// frequency / presence penalties (count: occurrences of the id in the window; both skipped for an empty window, libfalcon.cpp:3281-3336)
FQ_HD float fq_penalize(float v, bool bias_on, float bias, int count, float penalty, float alpha_f, float alpha_p) {
    if (bias_on) v += bias;
    if (count > 0) {
        if (penalty != 1.0f) v = v <= 0 ? v * penalty : v / penalty;
        if (alpha_f != 0.0f || alpha_p != 0.0f) v -= float(count) * alpha_f + float(count > 0) * alpha_p;
    }
    return v;
}

// ---- sort key: value descending, then id ascending (the documented tie rule) == the 64-bit key descending
FQ_HD uint32_t fq_fkey(float v) { const uint32_t u = fq_f2u(v); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
FQ_HD float fq_fkey_inv(uint32_t k) { return fq_u2f((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
FQ_HD uint64_t fq_sort_key(float v, int id) { return ((uint64_t) fq_fkey(v) << 32) | (uint64_t)(0xffffffffu - (uint32_t) id); }
FQ_HD float fq_key_val(uint64_t k) { return fq_fkey_inv((uint32_t)(k >> 32)); }
FQ_HD int fq_key_id(uint64_t k) { return (int)(0xffffffffu - (uint32_t) k); }

// ---- the chain's tail on the top-k candidates, sorted (val(i): i-th value, descending), temp > 0:
// top-p (llama_sample_top_p, min_keep 1), temperature, llama_sample_token's softmax and discrete_distribution draw.
// Returns the drawn position in [0, n).
template <class V>
FQ_HD int fq_sample_tail(V & val, int n, float top_p, float temp, uint32_t * mt, int * mti) {
    if (top_p < 1.0f) {
        const float m = val(0);
        float sum = 0.0f;
        for (int i = 0; i < n; ++i) {
            const float e = fq_expf(val(i) - m);
            if (fq_negligible_f(e, sum)) break;
            sum += e;
        }
        float cum = 0.0f;
        for (int i = 0; i < n; ++i) {
            const float p = fq_expf(val(i) - m) / sum;
            if (fq_negligible_f(p, cum)) {                  // cum is final: the first index >= 1 from here on crosses, or none does
                if (cum > top_p) n = i < 1 ? 1 : i;
                break;
            }
            cum += p;
            if (cum > top_p && i >= 1) { n = i; break; }
        }
    }
    const float mt0 = val(0) / temp;
    float sum = 0.0f;
    for (int i = 0; i < n; ++i) {
        const float e = fq_expf(val(i) / temp - mt0);
        if (fq_negligible_f(e, sum)) break;
        sum += e;
    }
    if (n < 2) return 0;                                    // discrete_distribution of one weight: index 0, no draw
    double sd = 0.0;
    for (int i = 0; i < n; ++i) {
        const double p = (double)(fq_expf(val(i) / temp - mt0) / sum);
        if (fq_negligible_d(p, sd)) break;
        sd += p;
    }
    const double u = fq_canonical(mt, mti);
    double c = 0.0;
    for (int i = 0; i < n - 1; ++i) {
        const double q = (double)(fq_expf(val(i) / temp - mt0) / sum) / sd;
        if (fq_negligible_d(q, c)) return n - 1;           // the partial sums stay below u up to the last entry, which is 1
        c += q;
        if (c >= u) return i;
    }
    return n - 1;
}
