// Host-side check of ggllm.cpp_amd/csrc/fq_sample.h (the exact header the device sampler compiles): its expf against the
// host libm's, its mt19937 against std::mt19937, and the whole chain (penalties, top-k sort, tail) for the test to compare
// with the reference's own sampling functions.
#include "fq_sample.h"
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <random>
#include <thread>
#include <vector>

extern "C" {

// every float in [lo, hi] (given as bit patterns of NON-POSITIVE floats, hi_bits >= lo_bits means more negative):
// number of inputs where fq_expf and libm expf differ in any bit; *first_bad: the first such input's bits
long long sample_expf_mismatches(uint32_t from_bits, uint32_t to_bits, int n_threads, uint32_t * first_bad) {
    std::atomic<long long> bad{0};
    std::atomic<uint32_t> first{0xffffffffu};
    std::vector<std::thread> th;
    const uint64_t span = (uint64_t) to_bits - from_bits + 1;
    for (int t = 0; t < n_threads; ++t)
        th.emplace_back([&, t] {
            const uint64_t b0 = from_bits + span * t / n_threads, b1 = from_bits + span * (t + 1) / n_threads;
            long long nb = 0;
            for (uint64_t b = b0; b < b1; ++b) {
                const float x = fq_u2f((uint32_t) b);
                if (fq_f2u(fq_expf(x)) != fq_f2u(expf(x))) {
                    ++nb;
                    uint32_t f = first.load();
                    while ((uint32_t) b < f && !first.compare_exchange_weak(f, (uint32_t) b)) {}
                }
            }
            bad += nb;
        });
    for (auto & x : th) x.join();
    *first_bad = first.load();
    return bad.load();
}

// n draws of fq_mt_next against std::mt19937 seeded with the same value: number of differing draws
int sample_mt_mismatches(uint32_t seed, int n) {
    std::mt19937 ref(seed);
    uint32_t mt[FQ_MT_N]; int mti;
    fq_mt_seed(mt, &mti, seed);
    int bad = 0;
    for (int i = 0; i < n; ++i) bad += fq_mt_next(mt, &mti) != (uint32_t) ref();
    return bad;
}

void sample_mt_seed(uint32_t * mt, int * mti, uint32_t seed) { fq_mt_seed(mt, mti, seed); }

double sample_canonical(uint32_t * mt, int * mti) { return fq_canonical(mt, mti); }

// the whole chain on one row: logit bias, penalties over the window, greedy (temp <= 0) or top-k (sorted by value desc,
// id asc) + fq_sample_tail. mt / mti: the row's generator, advanced.
int sample_chain(const float * logits, int n_vocab, float temp, int top_k, float top_p, float penalty, float alpha_f, float alpha_p,
                 const int32_t * window, int n_window, int n_bias, const int32_t * bias_id, const float * bias, uint32_t * mt, int * mti) {
    std::vector<float> v(n_vocab);
    for (int i = 0; i < n_vocab; ++i) {
        int count = 0;
        for (int j = 0; j < n_window; ++j) count += window[j] == i;
        bool bon = false; float b = 0.0f;
        for (int j = 0; j < n_bias; ++j) if (bias_id[j] == i) { bon = true; b = bias[j]; }
        v[i] = fq_penalize(logits[i], bon, b, count, penalty, alpha_f, alpha_p);
    }
    if (temp <= 0) {
        int best = 0;
        for (int i = 1; i < n_vocab; ++i) if (v[i] > v[best]) best = i;
        return best;
    }
    int k = top_k <= 0 ? n_vocab : top_k;
    k = std::max(k, 1); k = std::min(k, n_vocab);
    std::vector<uint64_t> keys(n_vocab);
    for (int i = 0; i < n_vocab; ++i) keys[i] = fq_sort_key(v[i], i);
    std::sort(keys.begin(), keys.end(), [](uint64_t a, uint64_t b) { return a > b; });
    auto val = [&](int i) { return fq_key_val(keys[i]); };
    const int pos = fq_sample_tail(val, k, top_p, temp, mt, mti);
    return fq_key_id(keys[pos]);
}

}
