// fq_sample_chain.h -- the rest of falcon_main's sampling branches (examples/falcon/falcon_main.cpp:960-981), restated once
// for the device sampler (kernels_sample.hip) and a host test (tests/test_sample_chain_cpu.py compiles this header with g++):
// the two stages fq_sample.h treats as off -- tail-free (libfalcon.cpp:3154-3203) and typical (3206-3267) -- and mirostat 1
// and 2 (3342-3431).
//
// What must be reproduced bit for bit besides fq_sample.h's list:
//   * the host libm's logf, log2f and powf (glibc's flt-32 e_logf.c, e_log2f.c, e_powf.c in the FMA variants its ifunc
//     selects: every a * b + c of their double arithmetic fused) -- fq_logf, fq_log2f, fq_powf. A NaN result is a NaN here
//     too; its sign and payload are the hardware's;
//   * the f32 sums, sequential in candidate order: the softmaxes, tail-free's derivative sum, typical's entropy and
//     cumulative sums, mirostat 1's two regressions sums;
//   * int(k) of mirostat 1 by x86's rule (cvttss2si: NaN and out of range give INT_MIN).
//
// Tail-free and typical run on at most FQ_CHAIN_MAX candidates (the top-k survivors of the LDS form), through arrays the caller
// owns (LDS on the device): no early exits -- after typical the candidates are ordered by shifted score, the logits are
// no longer descending (the softmax that follows subtracts data[0].logit, which is not the maximum: expf sees positive
// arguments), and fq_sample.h's fq_negligible_* cuts do not hold. Mirostat runs on the whole sorted vocabulary, where they do.
//
// Tie rule where the reference's std::sort leaves the order open: typical orders by (score ascending, position in logit
// order ascending) == the 64-bit fq_typical_key ascending; NaN scores (a probability of 0) sort last.
#pragma once
#include "fq_sample.h"

#define FQ_CHAIN_MAX 1024           // candidates tail-free and typical take
#define FQ_MIROSTAT_M 100           // falcon_main.cpp:966

// {invc, logc} of the 16 sub-intervals of [0x1.66p-1, 0x1.66p0): logf's (logc = ln c) and log2f's / powf's (logc = log2 c)
FQ_HD double fq_log_invc(int i) {
    const double T[16] = { 0x1.661ec79f8f3bep+0, 0x1.571ed4aaf883dp+0, 0x1.49539f0f010bp+0, 0x1.3c995b0b80385p+0, 0x1.30d190c8864a5p+0, 0x1.25e227b0b8eap+0,
                           0x1.1bb4a4a1a343fp+0, 0x1.12358f08ae5bap+0, 0x1.0953f419900a7p+0, 0x1p+0, 0x1.e608cfd9a47acp-1, 0x1.ca4b31f026aap-1,
                           0x1.b2036576afce6p-1, 0x1.9c2d163a1aa2dp-1, 0x1.886e6037841edp-1, 0x1.767dcf5534862p-1 };
    return T[i];
}
FQ_HD double fq_log_lnc(int i) {
    const double T[16] = { -0x1.57bf7808caadep-2, -0x1.2bef0a7c06ddbp-2, -0x1.01eae7f513a67p-2, -0x1.b31d8a68224e9p-3, -0x1.6574f0ac07758p-3, -0x1.1aa2bc79c81p-3,
                           -0x1.a4e76ce8c0e5ep-4, -0x1.1973c5a611cccp-4, -0x1.252f438e10c1ep-5, 0x0p+0, 0x1.aa5aa5df25984p-5, 0x1.c5e53aa362eb4p-4,
                           0x1.526e57720db08p-3, 0x1.bc2860d22477p-3, 0x1.1058bc8a07ee1p-2, 0x1.4043057b6ee09p-2 };
    return T[i];
}
FQ_HD double fq_log_log2c(int i) {
    const double T[16] = { -0x1.efec65b963019p-2, -0x1.b0b6832d4fca4p-2, -0x1.7418b0a1fb77bp-2, -0x1.39de91a6dcf7bp-2, -0x1.01d9bf3f2b631p-2, -0x1.97c1d1b3b7afp-3,
                           -0x1.2f9e393af3c9fp-3, -0x1.960cbbf788d5cp-4, -0x1.a6f9db6475fcep-5, 0x0p+0, 0x1.338ca9f24f53dp-4, 0x1.476a9543891bap-3,
                           0x1.e840b4ac4e4d2p-3, 0x1.40645f0c6651cp-2, 0x1.88e9c2c1b9ff8p-2, 0x1.ce0a44eb17bccp-2 };
    return T[i];
}

// glibc logf (sysdeps/ieee754/flt-32/e_logf.c, LOGF_TABLE_BITS 4)
FQ_HD float fq_logf(float x) {
    const double Ln2 = 0x1.62e42fefa39efp-1, A0 = -0x1.00ea348b88334p-2, A1 = 0x1.5575b0be00b6ap-2, A2 = -0x1.ffffef20a4123p-2;
    uint32_t ix = fq_f2u(x);
    if (ix == 0x3f800000u) return 0.0f;
    if (ix - 0x00800000u >= 0x7f800000u - 0x00800000u) {    // x < 0x1p-126, inf or nan
        if (ix * 2u == 0u) return -INFINITY;
        if (ix == 0x7f800000u) return x;
        if ((ix & 0x80000000u) || ix * 2u >= 0xff000000u) return (x - x) / (x - x);
        ix = fq_f2u(x * 0x1p23f);                           // subnormal: normalise
        ix -= 23u << 23;
    }
    const uint32_t tmp = ix - 0x3f330000u;
    const int i = (int)((tmp >> 19) % 16u);
    const int k = (int32_t) tmp >> 23;
    const uint32_t iz = ix - (tmp & 0xff800000u);
    const double z = (double) fq_u2f(iz);
    const double r = fma(z, fq_log_invc(i), -1.0);          // log(x) = log1p(z/c - 1) + log(c) + k ln2
    const double y0 = fma((double) k, Ln2, fq_log_lnc(i));
    const double r2 = r * r;
    double y = fma(A1, r, A2);
    y = fma(A0, r2, y);
    y = fma(y, r2, y0 + r);
    return (float) y;
}

// glibc log2f (e_log2f.c, LOG2F_TABLE_BITS 4)
FQ_HD float fq_log2f(float x) {
    const double A0 = -0x1.712b6f70a7e4dp-2, A1 = 0x1.ecabf496832ep-2, A2 = -0x1.715479ffae3dep-1, A3 = 0x1.715475f35c8b8p0;
    uint32_t ix = fq_f2u(x);
    if (ix == 0x3f800000u) return 0.0f;
    if (ix - 0x00800000u >= 0x7f800000u - 0x00800000u) {
        if (ix * 2u == 0u) return -INFINITY;
        if (ix == 0x7f800000u) return x;
        if ((ix & 0x80000000u) || ix * 2u >= 0xff000000u) return (x - x) / (x - x);
        ix = fq_f2u(x * 0x1p23f);
        ix -= 23u << 23;
    }
    const uint32_t tmp = ix - 0x3f330000u;
    const int i = (int)((tmp >> 19) % 16u);
    const uint32_t top = tmp & 0xff800000u;
    const uint32_t iz = ix - top;
    const int k = (int32_t) tmp >> 23;
    const double z = (double) fq_u2f(iz);
    const double r = fma(z, fq_log_invc(i), -1.0);          // log2(x) = log1p(z/c - 1)/ln2 + log2(c) + k
    const double y0 = fq_log_log2c(i) + (double) k;
    const double r2 = r * r;
    double y = fma(A1, r, A2);
    y = fma(A0, r2, y);
    const double p = fma(A3, r, y0);
    y = fma(y, r2, p);
    return (float) y;
}

// glibc powf (e_powf.c, POWF_LOG2_TABLE_BITS 4, POWF_SCALE_BITS 0; exp2f's table is fq_expf's)
FQ_HD int fq_pow_checkint(uint32_t iy) {                    // 0: not an integer, 1: odd, 2: even
    const int e = (int)(iy >> 23 & 0xff);
    if (e < 0x7f) return 0;
    if (e > 0x7f + 23) return 2;
    if (iy & ((1u << (0x7f + 23 - e)) - 1u)) return 0;
    if (iy & (1u << (0x7f + 23 - e))) return 1;
    return 2;
}
FQ_HD bool fq_pow_zeroinfnan(uint32_t ix) { return 2u * ix - 1u >= 2u * 0x7f800000u - 1u; }
FQ_HD bool fq_pow_snan(uint32_t ix) { return 2u * (ix ^ 0x00400000u) > 2u * 0x7fc00000u; }
FQ_HD float fq_powf(float x, float y) {
    const uint64_t T[32] = {
        0x3ff0000000000000ull, 0x3fefd9b0d3158574ull, 0x3fefb5586cf9890full, 0x3fef9301d0125b51ull, 0x3fef72b83c7d517bull, 0x3fef54873168b9aaull,
        0x3fef387a6e756238ull, 0x3fef1e9df51fdee1ull, 0x3fef06fe0a31b715ull, 0x3feef1a7373aa9cbull, 0x3feedea64c123422ull, 0x3feece086061892dull,
        0x3feebfdad5362a27ull, 0x3feeb42b569d4f82ull, 0x3feeab07dd485429ull, 0x3feea47eb03a5585ull, 0x3feea09e667f3bcdull, 0x3fee9f75e8ec5f74ull,
        0x3feea11473eb0187ull, 0x3feea589994cce13ull, 0x3feeace5422aa0dbull, 0x3feeb737b0cdc5e5ull, 0x3feec49182a3f090ull, 0x3feed503b23e255dull,
        0x3feee89f995ad3adull, 0x3feeff76f2fb5e47ull, 0x3fef199bdd85529cull, 0x3fef3720dcef9069ull, 0x3fef5818dcfba487ull, 0x3fef7c97337b9b5full,
        0x3fefa4afa2a490daull, 0x3fefd0765b6e4540ull };
    const double A0 = 0x1.27616c9496e0bp-2, A1 = -0x1.71969a075c67ap-2, A2 = 0x1.ec70a6ca7baddp-2, A3 = -0x1.7154748bef6c8p-1, A4 = 0x1.71547652ab82bp0;
    const double C0 = 0x1.c6af84b912394p-5, C1 = 0x1.ebfce50fac4f3p-3, C2 = 0x1.62e42ff0c52d6p-1, SHIFT = 0x1.8p+47;
    uint64_t sign_bias = 0;
    uint32_t ix = fq_f2u(x);
    const uint32_t iy = fq_f2u(y);
    if (ix - 0x00800000u >= 0x7f800000u - 0x00800000u || fq_pow_zeroinfnan(iy)) {
        if (fq_pow_zeroinfnan(iy)) {
            if (2u * iy == 0u) return fq_pow_snan(ix) ? x + y : 1.0f;
            if (ix == 0x3f800000u) return fq_pow_snan(iy) ? x + y : 1.0f;
            if (2u * ix > 2u * 0x7f800000u || 2u * iy > 2u * 0x7f800000u) return x + y;
            if (2u * ix == 2u * 0x3f800000u) return 1.0f;
            if ((2u * ix < 2u * 0x3f800000u) == !(iy & 0x80000000u)) return 0.0f;      // |x| < 1 && y == inf, or |x| > 1 && y == -inf
            return y * y;
        }
        if (fq_pow_zeroinfnan(ix)) {
            float x2 = x * x;
            bool neg = false;
            if ((ix & 0x80000000u) && fq_pow_checkint(iy) == 1) { x2 = -x2; neg = true; }
            if (2u * ix == 0u && (iy & 0x80000000u)) return (neg ? -1.0f : 1.0f) / 0.0f;
            return (iy & 0x80000000u) ? 1 / x2 : x2;
        }
        if (ix & 0x80000000u) {                             // finite x < 0
            const int yint = fq_pow_checkint(iy);
            if (yint == 0) return (x - x) / (x - x);
            if (yint == 1) sign_bias = 1ull << (5 + 11);
            ix &= 0x7fffffffu;
        }
        if (ix < 0x00800000u) {                             // subnormal x: normalise
            ix = fq_f2u(x * 0x1p23f);
            ix &= 0x7fffffffu;
            ix -= 23u << 23;
        }
    }
    // log2(x) in double
    const uint32_t tmp = ix - 0x3f330000u;
    const int i = (int)((tmp >> 19) % 16u);
    const uint32_t top = tmp & 0xff800000u;
    const uint32_t iz = ix - top;
    const int k = (int32_t) top >> 23;
    const double z = (double) fq_u2f(iz);
    const double r = fma(z, fq_log_invc(i), -1.0);
    const double y0 = fq_log_log2c(i) + (double) k;
    const double r2 = r * r;
    double l = fma(A0, r, A1);
    const double p = fma(A2, r, A3);
    const double r4 = r2 * r2;
    double q = fma(A4, r, y0);
    q = fma(p, r2, q);
    l = fma(l, r4, q);
    const double ylogx = (double) y * l;
    if ((fq_d2u(ylogx) >> 47 & 0xffff) >= fq_d2u(126.0) >> 47) {      // |y log2 x| >= 126
        const float big = 0x1p97f, tiny = 0x1p-95f, may = 0x1.4p-75f;
        if (ylogx > 0x1.fffffffd1d571p+6) return (sign_bias ? -big : big) * big;
        if (ylogx <= -150.0) return (sign_bias ? -tiny : tiny) * tiny;
        if (ylogx < -149.0) return (sign_bias ? -may : may) * may;
    }
    // exp2(ylogx)
    double kd = ylogx + SHIFT;
    const uint64_t ki = fq_d2u(kd);
    kd -= SHIFT;
    const double rr = ylogx - kd;
    uint64_t t = T[ki % 32];
    t += (ki + sign_bias) << 47;
    const double s = fq_u2d(t);
    const double zz = fma(C0, rr, C1);
    const double rr2 = rr * rr;
    double e = fma(C2, rr, 1.0);
    e = fma(zz, rr2, e);
    e = e * s;
    return (float) e;
}

// int(x) as x86's cvttss2si does it: NaN and anything outside int's range give INT_MIN
FQ_HD int fq_f2i_x86(float x) { return (x >= -2147483648.0f && x < 2147483648.0f) ? (int) x : (int) 0x80000000u; }

// ---- llama_sample_softmax over n candidates in the order given (data[0] need not hold the maximum): p[i]
template <class V>
FQ_HD void fq_chain_softmax(V & val, int n, float * p) {
    const float m = val(0);
    float sum = 0.0f;
    for (int i = 0; i < n; ++i) { p[i] = fq_expf(val(i) - m); sum += p[i]; }
    for (int i = 0; i < n; ++i) p[i] /= sum;
}

// ---- llama_sample_tail_free (min_keep 1) on n <= FQ_CHAIN_MAX candidates sorted by logit; p: n floats of scratch. Returns the new n.
// The reference's `abs(second_derivatives[i])` resolves to the INTEGER abs in its build (the compiled function converts with
// cvttss2si, negates, converts back): every second difference of probabilities truncates to 0 unless it is +-1, their sum is
// 0, the normalised values are 0 / 0 = NaN, no running sum exceeds z and nothing is cut -- except on a row whose
// probabilities are exactly {1, 0, 0, 0, ...}. Restated as compiled.
template <class V>
FQ_HD int fq_tail_free(V & val, int n, float z, float * p) {
    if (z >= 1.0f || n <= 2) return n;
    fq_chain_softmax(val, n, p);
    for (int i = 0; i < n - 1; ++i) p[i] = p[i] - p[i + 1];            // first differences (p[i + 1] is still a probability)
    for (int i = 0; i < n - 2; ++i) {                                   // second (p[i + 1] is still a first difference), abs(int)
        const int d = fq_f2i_x86(p[i] - p[i + 1]);
        p[i] = float(d < 0 ? (int)(0u - (unsigned) d) : d);
    }
    float sum = 0.0f;
    for (int i = 0; i < n - 2; ++i) sum += p[i];
    float cum = 0.0f;
    for (int i = 0; i < n - 2; ++i) {
        cum += p[i] / sum;
        if (cum > z && i >= 1) return i;
    }
    return n;
}

// ---- llama_sample_typical (min_keep 1), first half: the probabilities p[i] and, per candidate, the key that orders it
// (shifted score, then position). Sort the keys ascending, then fq_typical_cut.
FQ_HD uint64_t fq_typical_key(float score, int pos) { return ((uint64_t)(fq_f2u(score) & 0x7fffffffu) << 32) | (uint32_t) pos; }
FQ_HD int fq_typical_pos(uint64_t key) { return (int)(uint32_t) key; }
template <class V>
FQ_HD void fq_typical_scores(V & val, int n, float * p, uint64_t * key) {
    fq_chain_softmax(val, n, p);
    float entropy = 0.0f;
    for (int i = 0; i < n; ++i) entropy += -p[i] * fq_logf(p[i]);
    for (int i = 0; i < n; ++i) key[i] = fq_typical_key(fabsf(-fq_logf(p[i]) - entropy), i);
}
// second half: the candidates kept, in key order (the cut at cum > typical_p && i >= 0)
FQ_HD int fq_typical_cut(const float * p, const uint64_t * key, int n, float typical_p) {
    float cum = 0.0f;
    for (int i = 0; i < n; ++i) {
        cum += p[fq_typical_pos(key[i])];
        if (cum > typical_p) return i + 1;
    }
    return n;
}

// ---- std::discrete_distribution over the n probabilities prob(i) (bits/random.tcc, as fq_sample_tail): the drawn position
template <class P>
FQ_HD int fq_chain_draw(P & prob, int n, uint32_t * mt, int * mti) {
    if (n < 2) return 0;
    double sd = 0.0;
    for (int i = 0; i < n; ++i) sd += (double) prob(i);
    const double u = fq_canonical(mt, mti);
    double c = 0.0;
    for (int i = 0; i < n - 1; ++i) {
        c += (double) prob(i) / sd;
        if (c >= u) return i;
    }
    return n - 1;
}

// ---- the default chain's tail behind tail-free / typical: top-p (min_keep 1), temperature, llama_sample_token, on n <= FQ_CHAIN_MAX
// candidates in ANY order (fq_sample_tail without its cuts). p: n floats of scratch. Returns the drawn position.
template <class V>
FQ_HD int fq_chain_tail(V & val, int n, float top_p, float temp, float * p, uint32_t * mt, int * mti) {
    if (top_p < 1.0f) {
        fq_chain_softmax(val, n, p);
        float cum = 0.0f;
        for (int i = 0; i < n; ++i) {
            cum += p[i];
            if (cum > top_p && i >= 1) { n = i; break; }
        }
    }
    const float mt0 = val(0) / temp;
    float sum = 0.0f;
    for (int i = 0; i < n; ++i) { p[i] = fq_expf(val(i) / temp - mt0); sum += p[i]; }
    for (int i = 0; i < n; ++i) p[i] /= sum;
    auto prob = [&](int i) { return p[i]; };
    return fq_chain_draw(prob, n, mt, mti);
}

// ---- mirostat 1 / 2 (llama_sample_token_mirostat with m = FQ_MIROSTAT_M, llama_sample_token_mirostat_v2) behind
// llama_sample_temperature, on the whole vocabulary sorted by penalised logit, descending (val(i): BEFORE the division by
// temp, which is monotone: sort first, divide when read). n_vocab: the model's (mirostat 1's N). *mu: the row's state,
// updated. *kept (optional): the candidates the draw ran over. *odd (optional, the host test's): set when a logf / log2f
// met a probability that is not a normal number. Returns the drawn position.
template <class V>
FQ_HD int fq_mirostat(V & val, int n, int version, float temp, float tau, float eta, int n_vocab, float * mu, uint32_t * mt, int * mti, int * kept, int * odd) {
    const float m = val(0) / temp;
    float sum = 0.0f;
    for (int i = 0; i < n; ++i) {
        const float e = fq_expf(val(i) / temp - m);
        if (fq_negligible_f(e, sum)) break;
        sum += e;
    }
    int k = n;
    if (version == 2) {
        for (int i = 0; i < n; ++i) {
            const float p = fq_expf(val(i) / temp - m) / sum;
            if (odd && !(p >= 0x1p-126f)) *odd = 1;
            if (-fq_log2f(p) > *mu) { k = i; break; }
        }
        if (k == 0) k = 1;
    } else {
        float sum_ti_bi = 0.0f, sum_ti_sq = 0.0f;
        float p0 = fq_expf(val(0) / temp - m) / sum;
        for (int i = 0; i < FQ_MIROSTAT_M - 1 && i < n - 1; ++i) {
            const float p1 = fq_expf(val(i + 1) / temp - m) / sum;
            if (odd && !(p0 >= 0x1p-126f && p1 >= 0x1p-126f)) *odd = 1;
            const float t_i = fq_logf(float(i + 2) / float(i + 1));
            const float b_i = fq_logf(p0 / p1);
            sum_ti_bi += t_i * b_i;
            sum_ti_sq += t_i * t_i;
            p0 = p1;
        }
        const float s_hat = sum_ti_bi / sum_ti_sq;
        const float epsilon_hat = s_hat - 1;
        const float kf = fq_powf((epsilon_hat * fq_powf(2.0f, *mu)) / (1 - fq_powf(float(n_vocab), -epsilon_hat)), 1 / s_hat);
        k = fq_f2i_x86(kf);
        k = k < 1 ? 1 : k;
        k = k > n ? n : k;
    }
    if (kept) *kept = k;
    // the softmax over the k kept (llama_sample_token's repeats it), the draw, the update
    float sum2 = 0.0f;
    for (int i = 0; i < k; ++i) {
        const float e = fq_expf(val(i) / temp - m);
        if (fq_negligible_f(e, sum2)) break;
        sum2 += e;
    }
    int pos = 0;
    if (k >= 2) {
        double sd = 0.0;
        for (int i = 0; i < k; ++i) {
            const double p = (double)(fq_expf(val(i) / temp - m) / sum2);
            if (fq_negligible_d(p, sd)) break;
            sd += p;
        }
        const double u = fq_canonical(mt, mti);
        double c = 0.0;
        pos = k - 1;
        for (int i = 0; i < k - 1; ++i) {
            const double q = (double)(fq_expf(val(i) / temp - m) / sum2) / sd;
            if (fq_negligible_d(q, c)) break;               // the partial sums stay below u up to the last entry, which is 1
            c += q;
            if (c >= u) { pos = i; break; }
        }
    }
    const float px = fq_expf(val(pos) / temp - m) / sum2;
    if (odd && !(px >= 0x1p-126f)) *odd = 1;
    const float e = -fq_log2f(px) - tau;
    *mu = *mu - eta * e;
    return pos;
}
