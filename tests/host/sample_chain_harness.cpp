// Host-side check of ggllm.cpp_amd/csrc/fq_sample_chain.h (the exact header the device sampler compiles): its logf, log2f,
// powf (and expf on the positive arguments typical opens) against the host libm's, and the whole chain -- penalties, top-k
// sort, tail-free, typical, top-p, temperature, draw; mirostat 1 and 2 with their mu -- for the test to compare with the
// reference's own sampling functions. Every chain call also reports whether the row was ambiguous under the documented
// contract (a tie in logit or in typical's score among the kept candidates and the first one dropped, or a logf / log2f of
// a probability that is not a normal number).
#include "fq_sample_chain.h"
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <thread>
#include <vector>

static inline bool same_f(float a, float b) { return fq_f2u(a) == fq_f2u(b) || (a != a && b != b); }      // (a NaN's sign and payload are not compared)

template <class F>
static long long sweep(uint64_t from, uint64_t to, int n_threads, uint64_t * first_bad, F bad_at) {
    std::atomic<long long> bad{0};
    std::atomic<uint64_t> first{~0ull};
    std::vector<std::thread> th;
    const uint64_t span = to - from + 1;
    for (int t = 0; t < n_threads; ++t)
        th.emplace_back([&, t] {
            const uint64_t b0 = from + span / n_threads * t, b1 = t + 1 == n_threads ? to + 1 : from + span / n_threads * (t + 1);
            long long nb = 0;
            for (uint64_t b = b0; b < b1; ++b)
                if (bad_at(b)) {
                    ++nb;
                    uint64_t f = first.load();
                    while (b < f && !first.compare_exchange_weak(f, b)) {}
                }
            bad += nb;
        });
    for (auto & x : th) x.join();
    *first_bad = first.load();
    return bad.load();
}

static inline uint64_t mix64(uint64_t z) {                 // splitmix64
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

extern "C" {

// every float whose bits lie in [from_bits, to_bits]: inputs where fq_<fn> and libm's differ. fn: 0 logf, 1 log2f, 2 expf
long long chain_fn_mismatches(int fn, uint32_t from_bits, uint32_t to_bits, int n_threads, uint32_t * first_bad) {
    uint64_t first;
    const long long bad = sweep(from_bits, to_bits, n_threads, &first, [fn](uint64_t b) {
        const float x = fq_u2f((uint32_t) b);
        return fn == 0 ? !same_f(fq_logf(x), logf(x)) : fn == 1 ? !same_f(fq_log2f(x), log2f(x)) : !same_f(fq_expf(x), expf(x));
    });
    *first_bad = (uint32_t) first;
    return bad;
}

// powf(x, y) for every y whose bits lie in [from_bits, to_bits]
long long chain_powf_mismatches(float x, uint32_t from_bits, uint32_t to_bits, int n_threads, uint32_t * first_bad) {
    uint64_t first;
    const long long bad = sweep(from_bits, to_bits, n_threads, &first, [x](uint64_t b) {
        const float y = fq_u2f((uint32_t) b);
        return !same_f(fq_powf(x, y), powf(x, y));
    });
    *first_bad = (uint32_t) first;
    return bad;
}

// pair `index` of the pseudo-random sweep: x > 0 with an exponent in [2^-48, 2^48) -- beyond what epsilon_hat * 2^mu /
// (1 - N^-epsilon_hat) yields for mu <= 40 -- and any mantissa; y of either sign with |y| in [2^-12, 2^7) (1 / s_hat, -epsilon_hat, mu)
void chain_powf_pair(uint64_t seed, uint64_t index, float * x, float * y) {
    const uint64_t r = mix64(seed ^ mix64(index));
    const uint32_t ex = 127 - 48 + (uint32_t)((r >> 23) & 0xffff) % 96, ey = 127 - 12 + (uint32_t)((r >> 40) & 0xff) % 19;
    *x = fq_u2f((ex << 23) | (uint32_t)(r & 0x7fffff));
    *y = fq_u2f((uint32_t)(r >> 63) << 31 | (ey << 23) | (uint32_t)((r >> 48) & 0x7fff) << 8 | (uint32_t)(mix64(r) & 0xff));
}
long long chain_powf_random_mismatches(uint64_t seed, uint64_t count, int n_threads, uint64_t * first_bad) {
    return sweep(0, count - 1, n_threads, first_bad, [seed](uint64_t b) {
        float x, y;
        chain_powf_pair(seed, b, &x, &y);
        return !same_f(fq_powf(x, y), powf(x, y));
    });
}
int chain_powf_same(float x, float y) { return same_f(fq_powf(x, y), powf(x, y)); }
uint32_t chain_powf_bits(float x, float y) { return fq_f2u(fq_powf(x, y)); }
int chain_f2i(float x) { return fq_f2i_x86(x); }

void chain_mt_seed(uint32_t * mt, int * mti, uint32_t seed) { fq_mt_seed(mt, mti, seed); }

// One draw of the whole chain on one row. mirostat 0: logit bias, penalties, greedy (temp <= 0) or top-k, tail-free, typical,
// top-p, temperature, draw; 1 / 2: bias, penalties, temperature, mirostat (model_n_vocab: mirostat 1's N), *mu updated.
// *ambiguous is set (never cleared) when the row lies outside the contract. Returns the token, or -1 for parameters the
// restatement does not take (tail-free / typical on more than FQ_CHAIN_MAX candidates).
int chain_draw(const float * logits, int n_vocab, float temp, int top_k, float top_p, float tfs_z, float typical_p, int mirostat, float tau, float eta,
               int model_n_vocab, float penalty, float alpha_f, float alpha_p, const int32_t * window, int n_window, int n_bias, const int32_t * bias_id,
               const float * bias, uint32_t * mt, int * mti, float * mu, int * ambiguous) {
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
    std::vector<uint64_t> keys(n_vocab);
    for (int i = 0; i < n_vocab; ++i) keys[i] = fq_sort_key(v[i], i);
    std::sort(keys.begin(), keys.end(), [](uint64_t a, uint64_t b) { return a > b; });
    auto val = [&](int i) { return fq_key_val(keys[i]); };
    auto ties = [&](int upto, float div) {                 // among candidates [0, upto] (upto: the first one dropped, where there is one)
        for (int i = 0; i < upto && i + 1 < n_vocab; ++i) if (val(i) / div == val(i + 1) / div) *ambiguous = 1;
    };
    if (mirostat == 1 || mirostat == 2) {
        int kept = 0, odd = 0;
        const int pos = fq_mirostat(val, n_vocab, mirostat, temp, tau, eta, model_n_vocab, mu, mt, mti, &kept, &odd);
        if (odd) *ambiguous = 1;
        ties(kept, temp);
        return fq_key_id(keys[pos]);
    }
    int k = top_k <= 0 ? n_vocab : top_k;
    k = std::max(k, 1); k = std::min(k, n_vocab);
    ties(k, 1.0f);
    if (tfs_z >= 1.0f && typical_p >= 1.0f) return fq_key_id(keys[fq_sample_tail(val, k, top_p, temp, mt, mti)]);
    if (k > FQ_CHAIN_MAX) return -1;
    std::vector<float> p(k);
    std::vector<uint64_t> tk(k);
    int n = fq_tail_free(val, k, tfs_z, p.data());
    if (typical_p >= 1.0f) return fq_key_id(keys[fq_chain_tail(val, n, top_p, temp, p.data(), mt, mti)]);
    fq_typical_scores(val, n, p.data(), tk.data());
    for (int i = 0; i < n; ++i) if (!(p[i] >= 0x1p-126f)) *ambiguous = 1;
    std::sort(tk.begin(), tk.begin() + n);
    const int n2 = fq_typical_cut(p.data(), tk.data(), n, typical_p);
    for (int i = 0; i < n2 && i + 1 < n; ++i) if ((tk[i] >> 32) == (tk[i + 1] >> 32)) *ambiguous = 1;
    auto val2 = [&](int i) { return fq_key_val(keys[fq_typical_pos(tk[i])]); };
    const int pos = fq_chain_tail(val2, n2, top_p, temp, p.data(), mt, mti);
    return fq_key_id(keys[fq_typical_pos(tk[pos])]);
}

}
