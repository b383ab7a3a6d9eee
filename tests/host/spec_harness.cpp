// host build of ggllm.cpp_amd/csrc/fq_spec.h for tests/test_spec_cpu.py
#include "fq_spec.h"

extern "C" {
int spec_state_words() { return (int)(sizeof(fq_spec_state) / 4); }
int spec_lookup_seq(const int32_t * h, int n, int gmin, int gmax, int K, int32_t * drafts) { return fq_spec_lookup_seq(h, n, gmin, gmax, K, drafts); }
void spec_lookup_keys(const int32_t * h, int n, int gmin, int gmax, int K, int32_t * drafts) { fq_spec_lookup_keys(h, n, gmin, gmax, K, drafts); }
int spec_given_draft(const int32_t * q, int m, int s, int i) { return fq_spec_given_draft(q, m, s, i); }

// the passes of a run whose draws are truth[0..n_truth): per_pass[p] = draws of pass p; returns the number of passes.
// source 1: lookup over hist (capacity n_hist + n_truth), 2: the guess. pos / n_ctx as fq_spec_go_on takes them (n_ctx 0: off)
int spec_simulate(const int32_t * truth, int n_truth, int K, int source, int32_t * hist, int n_hist, int gmin, int gmax,
                  const int32_t * guess, int n_guess, int pos, int n_ctx, int32_t * per_pass) {
    int passes = 0, s = 0;
    int32_t d[FQ_SPEC_MAX_DRAFT];
    while (s < n_truth) {
        if (source == FQ_SPEC_LOOKUP) fq_spec_lookup_keys(hist, n_hist, gmin, gmax, K, d);
        else for (int i = 1; i <= K; ++i) d[i - 1] = fq_spec_given_draft(guess, n_guess, s, i);
        int j = 0;
        while (fq_spec_go_on(truth[s + j], j < K ? d[j] : -1, false, j, K, pos + s + j + 1, n_ctx, n_truth - (s + j + 1))) ++j;
        for (int i = 0; i <= j; ++i) hist[n_hist++] = truth[s + i];
        per_pass[passes++] = j + 1;
        s += j + 1;
    }
    return passes;
}
}
