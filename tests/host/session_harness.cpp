// session_harness.cpp -- TEST INFRASTRUCTURE: csrc/fq_session.h (and fq_sample.h's generator) behind a C ABI for tests/test_session_cpu.py (g++, host only).
#include "fq_sample.h"
#include "fq_session.h"

extern "C" {

int ss_overhead() { return FQ_SESSION_TENSOR_OVERHEAD; }

long ss_rng_format(const uint32_t * mt, int mti, char * dst) { return (long) fq_session_rng_format(mt, mti, dst); }
int ss_rng_parse(const char * s, long n, uint32_t * mt, int * mti) { return fq_session_rng_parse(s, (size_t) n, mt, mti); }

// fq_sample.h's std::mt19937(seed) after n_draws 32-bit draws
void ss_mt_after(uint32_t seed, int n_draws, uint32_t * mt, int * mti) {
    fq_mt_seed(mt, mti, seed);
    for (int i = 0; i < n_draws; ++i) (void) fq_mt_next(mt, mti);
}

// info: n_tokens, tokens offset, blob offset, logits capacity, logits size, logits offset, kv_ntok, K offset, V offset, blob bytes, generator position
int ss_parse(const uint8_t * p, long n, const int32_t * want_hp, long capacity, const int32_t * dims, int64_t * info, uint32_t * mt, int32_t * hp_out) {
    fq_session_hparams want;
    memcpy(&want, want_hp, sizeof want);
    fq_session_view s;
    const int rc = fq_session_parse(p, (size_t) n, want, (size_t) capacity, fq_session_dims{ dims[0], dims[1], dims[2] }, &s);
    if (rc) return rc;
    info[0] = s.n_tokens; info[1] = s.tokens - p; info[2] = (int64_t) s.state_off; info[3] = (int64_t) s.st.logits_cap; info[4] = (int64_t) s.st.logits_size;
    info[5] = s.st.logits - p; info[6] = s.st.kv_ntok; info[7] = s.st.k - p; info[8] = s.st.v - p; info[9] = (int64_t) s.st.n_bytes; info[10] = s.st.mti;
    memcpy(mt, s.st.mt, sizeof s.st.mt);
    memcpy(hp_out, &s.hp, sizeof s.hp);
    return 0;
}

long ss_file_bytes(long n_tokens, const int32_t * dims, long logits_cap, int kv_ntok) {
    return (long)(fq_session_header_bytes((size_t) n_tokens) + fq_state_bytes(fq_session_dims{ dims[0], dims[1], dims[2] }, (size_t) logits_cap, kv_ntok));
}

// k, v: the file's K and V sections as they lie (fq_session_kv_bytes each)
long ss_write(uint8_t * dst, const int32_t * hp, const int32_t * tokens, long n_tokens, const int32_t * dims, const uint32_t * mt, int mti, long logits_cap,
              const float * logits, long logits_size, int kv_ntok, const uint8_t * k, const uint8_t * v) {
    fq_session_hparams h;
    memcpy(&h, hp, sizeof h);
    const fq_session_dims d{ dims[0], dims[1], dims[2] };
    const size_t head = fq_session_write_header(dst, h, tokens, (uint32_t) n_tokens);
    uint8_t * kv = nullptr;
    const size_t body = fq_state_write(dst + head, d, mt, mti, (size_t) logits_cap, logits, (size_t) logits_size, kv_ntok, &kv);
    const size_t kvb = fq_session_kv_bytes(d, kv_ntok);
    if (kvb) { memcpy(kv, k, kvb); memcpy(kv + kvb, v, kvb); }
    return (long)(head + body);
}

}
