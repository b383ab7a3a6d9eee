// kernels_grammar.hip -- a constraint's index (csrc/fq_grammar.h): for every state of a byte automaton the bitmap of the tokens a row in
// that state may draw, built once on the device when the grammar is made. The sampler's MASK instantiations (kernels_sample_row.h)
// then read one row of it beside the logits row.
//
// k_grammar_index: a lane per token, a wave per 64-token word, FQ_GI_TILE states per lane in registers. The lane reads each byte of
// its token ONCE and steps all the tile's states through it (FQ_GI_TILE independent table loads in flight per byte); the wave's
// ballot over "allowed" is the index word, written by lane 0, which also adds its population count to the state's counter for the
// creation check. The transition table is read from global memory: a walk leaves the tile's states after one byte, so a tile's rows
// in LDS would serve only the first byte; the table of the WHOLE automaton (512 bytes a state: 32 KB at 64 states, 2 MB at 4096)
// stays in L2 for the launch.
#include "fq_device.h"
#include "hip_context.h"
#include "fq_grammar.h"
#include "../../include/ggml-hip-ops.h"

#include <string.h>
#include <vector>

static_assert(FQ_GRAMMAR_MAX_STATES == GGML_HIP_GRAMMAR_MAX_STATES && FQ_GRAMMAR_BAD_ARGS == GGML_HIP_GRAMMAR_BAD_ARGS && FQ_GRAMMAR_BAD_TRANS == GGML_HIP_GRAMMAR_BAD_TRANS &&
              FQ_GRAMMAR_DEAD_END == GGML_HIP_GRAMMAR_DEAD_END, "include/ggml-hip-ops.h restates csrc/fq_grammar.h's constants");

#define FQ_GI_TILE 16               // states per lane
#define FQ_GI_THREADS 256           // four words per workgroup

struct ggml_hip_grammar {
    int n_states, start, n_vocab, n_words, eos_id;
    uint16_t * trans; uint8_t * accept; uint64_t * allow;   // device: the table and the index
    uint8_t * pool; int32_t * offs;                          // device: its own copy of the vocabulary it was indexed with
    int bound;                                               // sampler rows that hold it
};

static thread_local int g_last_error = FQ_GRAMMAR_OK;

__global__ void __launch_bounds__(FQ_GI_THREADS) k_grammar_index(const uint16_t * __restrict__ trans, const uint8_t * __restrict__ accept, int n_states,
        const uint8_t * __restrict__ pool, const int32_t * __restrict__ offs, int n_vocab, int n_words, int eos_id,
        uint64_t * __restrict__ allow, int32_t * __restrict__ counts) {
    const int w = blockIdx.x * (FQ_GI_THREADS / 64) + (threadIdx.x >> 6);      // (wave-uniform)
    if (w >= n_words) return;
    const int lane = threadIdx.x & 63, t = w * 64 + lane, s0 = blockIdx.y * FQ_GI_TILE;
    const bool tok = t < n_vocab;
    const int o0 = tok ? offs[t] : 0, L = tok ? offs[t + 1] - o0 : 0;
    const bool eos = tok && t == eos_id;
    int st[FQ_GI_TILE];
#pragma unroll
    for (int k = 0; k < FQ_GI_TILE; ++k) st[k] = s0 + k < n_states ? s0 + k : 0;
    if (!eos)
        for (int i = 0; i < L; ++i) {
            const uint8_t b = pool[o0 + i];
#pragma unroll
            for (int k = 0; k < FQ_GI_TILE; ++k) st[k] = fq_grammar_step(trans, st[k], b);     // (state 0 steps to 0: the same as fq_grammar_walk's early end)
        }
#pragma unroll
    for (int k = 0; k < FQ_GI_TILE; ++k) {
        const int s = s0 + k;                               // (block-uniform)
        if (s >= n_states) break;
        const bool ok = tok && fq_grammar_allowed_after(accept, s, t, eos_id, L, st[k]);
        const uint64_t word = __ballot(ok);
        if (lane == 0) {
            allow[(int64_t) s * n_words + w] = word;
            if (word) atomicAdd(&counts[s], __popcll(word));
        }
    }
}

static void grammar_release(ggml_hip_grammar * g) {
    for (void * p : { (void *) g->trans, (void *) g->accept, (void *) g->allow, (void *) g->pool, (void *) g->offs }) if (p) HIP_CHECK(hipFree(p));
    delete g;
}

// the grammar over a vocabulary given as host arrays (dev == false) or as device arrays of n_vocab + 1 ascending offsets and their pool
ggml_hip_grammar * fq_grammar_make(const char * who, int n_vocab, const uint8_t * pool, const int32_t * offs, bool dev, const ggml_hip_dfa * dfa, int eos_id, int * bad_state) {
    int bad = -1;
    if (bad_state) *bad_state = -1;
    const int rc = !dfa || !offs ? FQ_GRAMMAR_BAD_ARGS : fq_grammar_check_table(dfa->n_states, dfa->start, dfa->trans, dfa->accept, n_vocab, eos_id, &bad);
    if (rc) {
        g_last_error = rc;
        if (bad_state) *bad_state = bad;
        if (rc == FQ_GRAMMAR_BAD_TRANS) fprintf(stderr, "%s: state %d of the automaton has a transition outside [0, %d) (or out of the dead state 0)\n", who, bad, dfa->n_states);
        else fprintf(stderr, "%s: needs 1 <= n_states <= %d, a start state and eos_id (-1: none) in range, the table and the accept flags\n", who, FQ_GRAMMAR_MAX_STATES);
        return nullptr;
    }
    hipStream_t st = fq_ctx().stream;
    ggml_hip_grammar * g = new ggml_hip_grammar();
    memset(g, 0, sizeof *g);
    g->n_states = dfa->n_states; g->start = dfa->start; g->n_vocab = n_vocab; g->n_words = fq_grammar_words(n_vocab); g->eos_id = eos_id;
    if (dev) {
        int32_t bytes = 0;
        HIP_CHECK(hipMemcpyAsync(&bytes, offs + n_vocab, 4, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        HIP_CHECK(hipMalloc((void **) &g->pool, (size_t)(bytes > 0 ? bytes : 1)));
        HIP_CHECK(hipMalloc((void **) &g->offs, ((size_t) n_vocab + 1) * 4));
        if (bytes > 0) HIP_CHECK(hipMemcpyAsync(g->pool, pool, (size_t) bytes, hipMemcpyDeviceToDevice, st));
        HIP_CHECK(hipMemcpyAsync(g->offs, offs, ((size_t) n_vocab + 1) * 4, hipMemcpyDeviceToDevice, st));
    } else if (fq_vocab_bytes_upload(who, pool, offs, n_vocab, &g->pool, &g->offs)) {
        g_last_error = FQ_GRAMMAR_BAD_ARGS;
        delete g;
        return nullptr;
    }
    const size_t S = (size_t) g->n_states;
    int32_t * counts = nullptr;
    HIP_CHECK(hipMalloc((void **) &g->trans, S * 512));
    HIP_CHECK(hipMalloc((void **) &g->accept, S));
    HIP_CHECK(hipMalloc((void **) &g->allow, S * g->n_words * 8));
    HIP_CHECK(hipMalloc((void **) &counts, S * 4));
    HIP_CHECK(hipMemcpyAsync(g->trans, dfa->trans, S * 512, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(g->accept, dfa->accept, S, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemsetAsync(counts, 0, S * 4, st));
    hipLaunchKernelGGL(k_grammar_index, dim3((unsigned)((g->n_words + FQ_GI_THREADS / 64 - 1) / (FQ_GI_THREADS / 64)), (unsigned)((g->n_states + FQ_GI_TILE - 1) / FQ_GI_TILE)),
                       dim3(FQ_GI_THREADS), 0, st, g->trans, g->accept, g->n_states, g->pool, g->offs, n_vocab, g->n_words, eos_id, g->allow, counts);
    std::vector<int32_t> h(S);
    HIP_CHECK(hipMemcpyAsync(h.data(), counts, S * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipFree(counts));
    if (const int rc2 = fq_grammar_check_counts(g->n_states, h.data(), &bad)) {
        g_last_error = rc2;
        if (bad_state) *bad_state = bad;
        fprintf(stderr, "%s: state %d of the automaton allows no token of this vocabulary (a row that reached it could draw nothing)\n", who, bad);
        grammar_release(g);
        return nullptr;
    }
    g_last_error = FQ_GRAMMAR_OK;
    return g;
}

// a sampler row's descriptor for g at `state` (-1: the start state): 0, or 1 when the state is out of range
int fq_grammar_row_of(const ggml_hip_grammar * g, int state, fq_grammar_row * out) {
    if (state == -1) state = g->start;
    if (state < 0 || state >= g->n_states) return 1;
    *out = fq_grammar_row{ g->trans, g->allow, g->pool, g->offs, g->n_words, g->eos_id, state, g->n_states };
    return 0;
}
int  fq_grammar_vocab(const ggml_hip_grammar * g) { return g->n_vocab; }
void fq_grammar_bind(ggml_hip_grammar * g, int by) { g->bound += by; }

// ------------------------------------------------------------------------------------------------ C ABI (include/ggml-hip-ops.h)
extern "C" ggml_hip_grammar * ggml_hip_grammar_create(int n_vocab, const uint8_t * pool_host, const int32_t * offsets_host, const ggml_hip_dfa * dfa, int eos_id, int * bad_state) {
    return fq_grammar_make("ggml-hip: grammar_create", n_vocab, pool_host, offsets_host, false, dfa, eos_id, bad_state);
}
extern "C" int ggml_hip_grammar_last_error(void) { return g_last_error; }

extern "C" int ggml_hip_grammar_free(ggml_hip_grammar * g) {
    if (!g) return 0;
    if (g->bound > 0) { fprintf(stderr, "ggml-hip: grammar_free: %d sampler rows still hold this grammar (ggml_hip_sampler_set_grammar(s, row, NULL, 0) first)\n", g->bound); return 1; }
    HIP_CHECK(hipStreamSynchronize(fq_ctx().stream));
    grammar_release(g);
    return 0;
}

extern "C" int ggml_hip_grammar_get_index(ggml_hip_grammar * g, int state0, int n, uint64_t * out) {
    if (!g || !out || state0 < 0 || n < 0 || (int64_t) state0 + n > g->n_states) { fprintf(stderr, "ggml-hip: grammar_get_index: states [%d, %d + %d) of %d\n", state0, state0, n, g ? g->n_states : 0); return 1; }
    hipStream_t st = fq_ctx().stream;
    if (n > 0) HIP_CHECK(hipMemcpyAsync(out, g->allow + (int64_t) state0 * g->n_words, (size_t) n * g->n_words * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}
