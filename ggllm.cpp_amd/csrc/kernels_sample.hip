// kernels_sample.hip -- falcon_main's default sampler chain on the device (examples/falcon/falcon_main.cpp:896-980):
// logit bias, repetition / frequency / presence penalties over the row's window, then greedy (temp <= 0) or top-k, top-p,
// temperature and the mt19937 draw of llama_sample_token (libfalcon.cpp:3038-3466). One workgroup samples one row and
// advances that row's loop state (window ring, generator, position, output slot), so the launch sits in a captured step.
//
// The penalties are applied as the row is read (an LDS bitmap of the ids with a bias entry or in the window, a hash table of
// the window's counts); the logits in HBM are never written. Top-k orders candidates by (value descending, id ascending):
//   k <= FQ_SK_SMALL_K  a radix select of the k-th 64-bit key (value bits, then id) over the row, the k survivors sorted in LDS;
//   larger k           a bitonic sort of the whole row's keys in a per-row HBM scratch buffer.
// The scalar tail (csrc/fq_sample.h) then runs on one lane over the sorted candidates.
//
// Stops (csrc/fq_stop.h, ggml_hip_sampler_set_stops): while any row has them, the launch also gets the rows' stop
// configuration, state and a `skip` word per row. A row whose state says it has ended leaves at the head of the launch (the
// whole workgroup: nothing of the row moves) and says so in its skip word; a row that draws runs fq_stop_draw on the lane that
// knows the token, before the position and the step counter advance.
//
// Stop strings (csrc/fq_stop_text.h, ggml_hip_sampler_set_stop_text): while any row has them the launch is a TEXT instantiation
// and also gets the rows' strings and byte rings and the vocabulary's bytes (a pool and n_vocab + 1 offsets in HBM). The row's
// strings, ring and byte count are staged into LDS at the head of the launch, under the row's read; behind fq_stop_draw the
// wave that holds the drawing lane matches the new token's bytes, a lane per byte (64 at a time for a longer token), each lane
// backwards through the token's own bytes and then the ring, and reduces to the smallest (byte, string). Without text stops
// the instantiations are the ones they always were.
//
// The end of the cache (fq_stop.h's fq_stop_context, ggml_hip_sampler_set_context_stop): while the limit is set every row has
// stops, and a row whose draw would move its position to the limit does not move; if no other rule ended it at that draw it
// ends with FQ_STOP_CONTEXT. The launch gets the limit as an argument (0: off) and writes the row's position and next token last.
//
// The other branches of falcon_main's sampling (csrc/fq_sample_chain.h, ggml_hip_sampler_set_row_ext): while any row uses
// tail-free, typical or mirostat the launch is the kernel's EXT instantiation, otherwise the one it always was. Tail-free and
// typical run on the LDS form's sorted survivors: one lane computes the probabilities and scores (the f32 sums are sequential
// by contract), the workgroup sorts typical's keys, one lane cuts and draws. Mirostat sorts the whole row in HBM as top_k <= 0
// does and keeps the row's mu in a device word the drawing lane updates -- no further launch, a captured step stays valid.
//
// Grammars (csrc/fq_grammar.h, ggml_hip_sampler_set_grammar; the index is kernels_grammar.hip's): while any row holds one the launch is a MASK
// instantiation and gets one descriptor per row -- the grammar's device arrays and the row's state word. A candidate whose bit is clear in the
// state's row of the index has the logit -inf behind bias and penalties (the index words are loaded with the logits, from HBM / L2); behind
// fq_stop_draw the drawing lane walks the drawn token's bytes and stores the new state. Rows without a grammar, and launches without MASK, draw
// what they always drew. k_verify_rows has no MASK instantiation: a verify pass on a row with a grammar is refused.
//
// Guidance (csrc/fq_guide.h, kernels_guide.hip, ggml_hip_sampler_set_guidance): while any row has a guide row, fq_launch_sample puts k_guide_mix in front on the
// same stream -- mixed[r] for every leader r -- and launches k_sample_rows_guided, the same row body with GUIDE on: a leader draws from mixed[r] in place of
// its logits row, with everything above unchanged behind that, and its drawing lane writes for the guide row what it writes for the row (token, position,
// output slot, step counter, skip word); a guide row's workgroup leaves at once -- nothing of the row is read or moved. Without pairs the launch is
// k_sample_rows, whose instantiations, arguments, registers and LDS are the ones they always were. k_verify_rows never sees guidance.
#include "fq_device.h"
#include "hip_context.h"
#include "fq_sample.h"
#include "fq_sample_chain.h"
#include "fq_stop.h"
#include "fq_stop_text.h"
#include "fq_grammar.h"
#include "fq_spec.h"
#include "../../include/ggml-hip-ops.h"

#include <math.h>
#include <string.h>
#include <vector>

static_assert(FQ_STOP_MAX_SEQS == GGML_HIP_STOP_MAX_SEQS && FQ_STOP_MAX_LEN == GGML_HIP_STOP_MAX_LEN && FQ_STOP_RUNNING == GGML_HIP_STOP_RUNNING &&
              FQ_STOP_BUDGET == GGML_HIP_STOP_BUDGET && FQ_STOP_CONTEXT == GGML_HIP_STOP_CONTEXT, "include/ggml-hip-ops.h restates csrc/fq_stop.h's constants");
static_assert(FQ_STOPT_MAX == GGML_HIP_STOP_TEXT_MAX && FQ_STOPT_MAX_LEN == GGML_HIP_STOP_TEXT_MAX_LEN && FQ_STOP_TEXT0 == GGML_HIP_STOP_TEXT0 &&
              FQ_STOP_TEXT0 == FQ_STOP_MAX_SEQS, "include/ggml-hip-ops.h restates csrc/fq_stop_text.h's constants; text reasons start where id reasons end");
static_assert(sizeof(ggml_hip_stop_text) == sizeof(fq_stopt_cfg) && sizeof(fq_stopt_cfg) % 4 == 0 && sizeof(fq_stopt_state) % 4 == 0, "a row's strings are the ABI's structure, staged as words");

static_assert(FQ_SPEC_MAX_DRAFT == GGML_HIP_SPEC_MAX_DRAFT && FQ_SPEC_LOOKUP == GGML_HIP_SPEC_LOOKUP && FQ_SPEC_GIVEN == GGML_HIP_SPEC_GIVEN, "include/ggml-hip-ops.h restates csrc/fq_spec.h's constants");

#define FQ_SK_THREADS 1024
#define FQ_SK_SMALL_K 1024          // top-k bound of the LDS form
#define FQ_SK_MAX_VOCAB 131072      // the id bitmap: 16 KB of LDS
#define FQ_SK_HASH 8192             // slots of the window's count table (64 KB of LDS)
#define FQ_SK_MAX_WINDOW 4096       // at most half the table's slots
#define FQ_SK_UNROLL 8              // row loads in flight per thread
#define FQ_SK_GBUF 256              // sorted keys the tail lane stages from HBM at a time (large-k form)
#define FQ_SK_MAX_VOCAB_BYTES (16 << 20)    // the vocabulary's byte pool (stop strings)

struct fq_sample_row {              // a row's parameters, in device memory (set by ggml_hip_sampler_set_row)
    float temp, top_p, penalty, alpha_f, alpha_p;
    int top_k, W, n_bias;
    int bias_id[FQ_SAMPLE_MAX_BIAS];
    float bias[FQ_SAMPLE_MAX_BIAS];
};

struct fq_sample_ext {              // what ggml_hip_sampler_set_row_ext adds to a row (off: tfs_z 1, typical_p 1, mirostat 0)
    float tfs_z, typical_p, tau, eta;
    int mirostat;
};
static bool ext_uses(const fq_sample_ext & x) { return !(x.tfs_z >= 1.0f) || !(x.typical_p >= 1.0f) || x.mirostat != 0; }

struct ggml_hip_sampler {
    int n_rows, n_vocab, n_ctx, np;         // np: the power of two >= n_vocab the large-k sort runs over
    fq_sample_row * rows;                   // [n_rows]
    int32_t * ring;                         // [n_rows][n_ctx]: the window (the last W tokens; order does not matter to the penalties)
    int * head;                             // [n_rows]: ring slot of the oldest entry
    uint32_t * mt;                          // [n_rows][625]: mt19937 state, index at [624]
    uint64_t * sort;                        // [n_rows][np]: large-k sort scratch
    int * steps;                            // [n_rows]: output slot counters of the model-level loops
    int32_t * tok;                          // [n_rows]: the last draw (ggml_hip_sampler_sample's staging)
    std::vector<int> W;                     // host copy of every row's window length (ggml_hip_sampler_copy_row)
    // tail-free, typical, mirostat: the rows' settings and mirostat's mu; the EXT kernel is launched only while ext_rows > 0
    fq_sample_ext * ext = nullptr;          // [n_rows]
    float * mu = nullptr;                   // [n_rows]
    std::vector<fq_sample_ext> ext_host;    // host copy of ext
    int ext_rows = 0;                       // rows that use one of the stages
    // stops: nothing exists until the first row gets some; the kernels are handed these only while stop_rows > 0
    fq_stop_cfg * stop_cfg = nullptr;       // [n_rows]
    fq_stop_state * stop_state = nullptr;   // [n_rows]
    int * stop_skip = nullptr;              // [n_rows]: 1 where the last launch skipped the row (the record launch reads it)
    std::vector<char> stop_on;              // host copy of every row's cfg.on (== stop_ids[row] || text_on[row])
    int stop_rows = 0;                      // rows with stops set
    // stop strings: the rows' arrays exist from the first row that gets some; the TEXT kernel is launched only while text_rows > 0
    fq_stopt_cfg * text_cfg = nullptr;      // [n_rows]
    fq_stopt_state * text_state = nullptr;  // [n_rows]
    std::vector<char> stop_ids, text_on;    // which of set_stops / set_stop_text turned the row's stops on
    int text_rows = 0;                      // rows with text stops set
    int ctx_limit = 0;                      // the end of the rows' caches (set_context_stop; 0: off): every row's stops are on while it is set
    uint8_t * vb_pool = nullptr;            // the vocabulary's bytes: token t is vb_pool[vb_offs[t] .. vb_offs[t + 1])
    int32_t * vb_offs = nullptr;            // [n_vocab + 1]
    bool vb_own = false;                    // set_vocab_bytes made them (a model's are shared by its contexts' samplers)
    // draft-and-verify (fq_spec.h): made by the first call that verifies; k_sample_rows' launches never see them
    int32_t * spec_draw = nullptr;          // [1]: the verify loop's last draw, handed from the drawing lane to the workgroup
    fq_spec_state * spec_state = nullptr;   // [1]: the operator-level verify's state (a context keeps its own)
    int32_t * spec_drafts = nullptr;        // [FQ_SPEC_MAX_DRAFT]: ... and its copy of the caller's drafts
    // grammars (fq_grammar.h): the rows' bindings and state words exist from the first row that gets one; the MASK kernel is launched only while gram_rows > 0
    fq_grammar_row * gram = nullptr;        // [n_rows]
    std::vector<ggml_hip_grammar *> gram_host;      // which grammar every row holds (null: none)
    int gram_rows = 0;                      // rows with a grammar
    // guidance (fq_guide.h): nothing exists until the first pair; the mix and the guided kernel are launched only while guide_pairs > 0
    int32_t * guide_of = nullptr;           // [n_rows]: the row's guide row (-1: none)
    int32_t * lead_of = nullptr;            // [n_rows]: the row's leader (-1: the row is no guide row)
    int32_t * mix_lead = nullptr;           // [n_rows]: k_guide_mix's leader of pair r -- r where the row leads, else -1
    float * guide_scale = nullptr;          // [n_rows]: the scale of the pair row r leads
    float * mixed = nullptr;                // [n_rows][mixed_stride]: the mixed row of the pair row r leads
    int64_t mixed_stride = 0;               // n_vocab rounded up to 4 floats: every mixed row is 16-byte aligned
    std::vector<int> guide_host, lead_host; // host copies
    std::vector<float> scale_host;
    int guide_pairs = 0;
};

struct sk_guide_args {                      // what a guided launch adds
    const int32_t * guide_of, * lead_of; const float * mixed; int64_t mixed_stride;
};
struct sk_text_args {                       // what a TEXT launch adds (all null otherwise)
    const fq_stopt_cfg * cfg; fq_stopt_state * state; const uint8_t * pool; const int32_t * offs;
};
#define FQ_SK_TEXT_CFG_W ((int)(sizeof(fq_stopt_cfg) / 4))
#define FQ_SK_TEXT_ST_W ((int)(sizeof(fq_stopt_state) / 4))
#define FQ_SK_TEXT_ST_T0 192                // the threads that stage the row's text state (behind those that stage its strings)
static_assert(FQ_SK_TEXT_CFG_W <= FQ_SK_TEXT_ST_T0 && FQ_SK_TEXT_ST_T0 + FQ_SK_TEXT_ST_W <= 1024, "one thread per staged word");

// LDS traffic inside one wave: the wave's LDS operations are served in program order, the fences keep the compiler from moving them
__device__ __forceinline__ void sk_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int sk_hash(int id) { return (int)(((uint32_t) id * 2654435761u) >> (32 - 13)); }

template <class V>
__device__ __forceinline__ void sk_bitonic_desc(V * a, int n, int tid) {      // n a power of two; a in LDS or (this workgroup's) HBM
    for (int k = 2; k <= n; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < n; i += FQ_SK_THREADS) {
                const int l = i ^ j;
                if (l > i) {
                    const V x = a[i], y = a[l];
                    if ((i & k) == 0 ? x < y : x > y) { a[i] = y; a[l] = x; }
                }
            }
            __syncthreads();
        }
}

struct sk_gsrc {                    // the tail's view of the sorted keys in HBM, staged through LDS
    const uint64_t * g; uint64_t * buf; int base, n;
    __device__ float operator()(int i) {
        if (i < base || i >= base + FQ_SK_GBUF) {
            base = i & ~(FQ_SK_GBUF - 1);
#pragma unroll 16
            for (int j = 0; j < FQ_SK_GBUF; ++j) buf[j] = base + j < n ? g[base + j] : 0;
        }
        return fq_key_val(buf[i - base]);
    }
};
struct sk_lsrc {
    const uint64_t * k;
    __device__ float operator()(int i) { return fq_key_val(k[i]); }
};

// token[row] = the row's draw; the row's window and generator advance. pos / steps+out (optional): pos[row] + 1, out[steps[row] * out_stride + row].
// stop_cfg / stop_state / stop_skip (all or none): a row that has ended is left as it is, skip[row] = 1
// EXT: ext[row]'s stages run (tail-free / typical behind the LDS form's top-k, or mirostat on the HBM sort, mug[row] its mu);
// without it neither array is read
// TEXT: the row's stop strings run behind fq_stop_draw (text: the rows' strings and rings, the vocabulary's bytes); without it text is not read
// ctx_limit > 0 (with pos and stops): a row whose draw moves it to ctx_limit ends (FQ_STOP_CONTEXT unless another rule ended it) and keeps pos[row] and token[row];
// drawn (optional): drawn[row] = the draw, also then
// (the body of one row as a function, for k_verify_rows: x = the logits row the draw is made from, row = the sampler row whose state draws and
// advances; false: the row had ended and nothing of it moved. Every thread of the workgroup calls it, with the same arguments.)
template <bool EXT, bool TEXT>
__device__ __forceinline__ bool sk_row(const float * __restrict__ xrow, const int row, int n, int np,
        const fq_sample_row * __restrict__ rows, int32_t * __restrict__ ring, int ring_cap, int * __restrict__ head, uint32_t * __restrict__ mtg,
        uint64_t * __restrict__ sortg, int32_t * __restrict__ token, int * __restrict__ pos, int * __restrict__ steps, int32_t * __restrict__ out, int out_stride,
        const fq_stop_cfg * __restrict__ stop_cfg, fq_stop_state * __restrict__ stop_state, int * __restrict__ stop_skip,
        const fq_sample_ext * __restrict__ ext, float * __restrict__ mug, sk_text_args text, int ctx_limit, int32_t * __restrict__ drawn) {
    const int tid = threadIdx.x;
    constexpr bool MASK = false;                            // (draft-and-verify has no grammars: falcon_hip_context_set_spec and ggml_hip_sampler_verify_rows refuse them)
    constexpr fq_grammar_row * gram = nullptr;
    constexpr bool GUIDE = false;                           // (... and never sees guidance)
    constexpr int sk_guide = -1;
#define SK_ROW_X xrow
#define SK_ROW_ENDED return false
#include "kernels_sample_row.h"
#undef SK_ROW_ENDED
#undef SK_ROW_X
    return true;
}

// MASK: gram[row] (fq_grammar.h) constrains the row's candidates to the tokens its state allows and moves the state with the draw; without it gram is not read
template <bool EXT, bool TEXT, bool MASK>
__global__ void __launch_bounds__(FQ_SK_THREADS) k_sample_rows(const float * __restrict__ logits, int64_t stride, int n, int np,
        const fq_sample_row * __restrict__ rows, int32_t * __restrict__ ring, int ring_cap, int * __restrict__ head, uint32_t * __restrict__ mtg,
        uint64_t * __restrict__ sortg, int32_t * __restrict__ token, int * __restrict__ pos, int * __restrict__ steps, int32_t * __restrict__ out, int out_stride,
        const fq_stop_cfg * __restrict__ stop_cfg, fq_stop_state * __restrict__ stop_state, int * __restrict__ stop_skip,
        const fq_sample_ext * __restrict__ ext, float * __restrict__ mug, sk_text_args text, int ctx_limit, int32_t * __restrict__ drawn,
        fq_grammar_row * __restrict__ gram) {
    const int row = blockIdx.x, tid = threadIdx.x;
    constexpr bool GUIDE = false;
    constexpr int sk_guide = -1;
#define SK_ROW_X (logits + (int64_t) row * stride)
#define SK_ROW_ENDED return
#include "kernels_sample_row.h"
#undef SK_ROW_ENDED
#undef SK_ROW_X
}

// k_sample_rows while some row has a guide row (gd: the pairs and the mixed rows k_guide_mix has just written): a guide row's workgroup leaves, a leader draws
// from its mixed row and writes its guide row's loop state with its own, every other row is k_sample_rows' row
template <bool EXT, bool TEXT, bool MASK>
__global__ void __launch_bounds__(FQ_SK_THREADS) k_sample_rows_guided(const float * __restrict__ logits, int64_t stride, int n, int np,
        const fq_sample_row * __restrict__ rows, int32_t * __restrict__ ring, int ring_cap, int * __restrict__ head, uint32_t * __restrict__ mtg,
        uint64_t * __restrict__ sortg, int32_t * __restrict__ token, int * __restrict__ pos, int * __restrict__ steps, int32_t * __restrict__ out, int out_stride,
        const fq_stop_cfg * __restrict__ stop_cfg, fq_stop_state * __restrict__ stop_state, int * __restrict__ stop_skip,
        const fq_sample_ext * __restrict__ ext, float * __restrict__ mug, sk_text_args text, int ctx_limit, int32_t * __restrict__ drawn,
        fq_grammar_row * __restrict__ gram, sk_guide_args gd) {
    const int row = blockIdx.x, tid = threadIdx.x;
    constexpr bool GUIDE = true;
    if (gd.lead_of[row] >= 0) return;                       // (the whole workgroup: a guide row draws nothing)
    const int sk_guide = gd.guide_of[row];
#define SK_ROW_X (sk_guide >= 0 ? gd.mixed + (int64_t) row * gd.mixed_stride : logits + (int64_t) row * stride)
#define SK_ROW_ENDED return
#include "kernels_sample_row.h"
#undef SK_ROW_ENDED
#undef SK_ROW_X
}

void fq_launch_sample(ggml_hip_sampler * s, int n_rows, const float * logits, int64_t row_stride, int32_t * token, int * pos, int * steps,
                      int32_t * out, int out_stride, hipStream_t st) {
    const bool ext = s->ext_rows > 0, txt = s->text_rows > 0;
    const sk_text_args text = txt ? sk_text_args{ s->text_cfg, s->text_state, s->vb_pool, s->vb_offs } : sk_text_args{ nullptr, nullptr, nullptr, nullptr };
    const bool mask = s->gram_rows > 0;
    auto kern = txt ? (ext ? k_sample_rows<true, true, false> : k_sample_rows<false, true, false>) : (ext ? k_sample_rows<true, false, false> : k_sample_rows<false, false, false>);
    if (mask) kern = txt ? (ext ? k_sample_rows<true, true, true> : k_sample_rows<false, true, true>) : (ext ? k_sample_rows<true, false, true> : k_sample_rows<false, false, true>);
    if (s->guide_pairs > 0) {                               // (no context stop here: set_guidance and set_context_stop refuse one another)
        fq_launch_guide(logits, row_stride, s->n_vocab, n_rows, s->mix_lead, s->guide_of, s->guide_scale, s->mixed, s->mixed_stride, nullptr, nullptr, st);
        auto kg = txt ? (ext ? k_sample_rows_guided<true, true, false> : k_sample_rows_guided<false, true, false>) : (ext ? k_sample_rows_guided<true, false, false> : k_sample_rows_guided<false, false, false>);
        if (mask) kg = txt ? (ext ? k_sample_rows_guided<true, true, true> : k_sample_rows_guided<false, true, true>) : (ext ? k_sample_rows_guided<true, false, true> : k_sample_rows_guided<false, false, true>);
        hipLaunchKernelGGL(kg, dim3((unsigned) n_rows), dim3(FQ_SK_THREADS), 0, st, logits, row_stride,
                           s->n_vocab, s->np, s->rows, s->ring, s->n_ctx, s->head, s->mt, s->sort, token, pos, steps, out, out_stride,
                           s->stop_rows > 0 ? s->stop_cfg : nullptr, s->stop_rows > 0 ? s->stop_state : nullptr, s->stop_rows > 0 ? s->stop_skip : nullptr,
                           s->ext, s->mu, text, 0, nullptr, mask ? s->gram : nullptr, sk_guide_args{ s->guide_of, s->lead_of, s->mixed, s->mixed_stride });
        return;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned) n_rows), dim3(FQ_SK_THREADS), 0, st, logits, row_stride,
                       s->n_vocab, s->np, s->rows, s->ring, s->n_ctx, s->head, s->mt, s->sort, token, pos, steps, out, out_stride,
                       s->stop_rows > 0 ? s->stop_cfg : nullptr, s->stop_rows > 0 ? s->stop_state : nullptr, s->stop_rows > 0 ? s->stop_skip : nullptr,
                       s->ext, s->mu, text, pos ? s->ctx_limit : 0, pos && s->ctx_limit > 0 && token != s->tok ? s->tok : nullptr, mask ? s->gram : nullptr);
}

// ------------------------------------------------------------------------------------------------ draft and verify (fq_spec.h)
struct sk_spec_args {
    fq_spec_state * st;                     // the sequence's state
    int32_t * history; int hist_cap;        // LOOKUP: prompt + draws (null: none kept)
    const int32_t * guess;                  // GIVEN
    int32_t * drafts;                       // [FQ_SPEC_MAX_DRAFT]: this pass's d_1..d_K on entry, the next pass's on exit (source OFF: left alone)
    int32_t * next_tok;                     // the model's token rows: [1 + i] = draft i + 1 of the next pass, 0 where there is none (null: not written)
    int32_t * draw;                         // [1] scratch
    int n_rows, source, ngram_min, ngram_max, n_ctx;
};

// the next pass's drafts, by the whole workgroup (red: one word per wave). LOOKUP: one max-reduction over the suffix keys of the history's ends
__device__ __forceinline__ void sk_make_drafts(int source, const int32_t * __restrict__ h, int hn, int gmin, int gmax, const int32_t * __restrict__ q, int nq, int at,
                                               int K, int32_t * __restrict__ drafts, int32_t * __restrict__ next_tok, long long * red) {
    const int tid = threadIdx.x;
    long long best = -1;
    if (source == FQ_SPEC_LOOKUP) {
        for (int e = tid; e <= hn - 2; e += (int) blockDim.x) { const long long k = fq_spec_suffix_key(h, hn, e, gmax); best = k > best ? k : best; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const long long ok = __shfl_xor(best, o); best = ok > best ? ok : best; }
        if ((tid & 63) == 0) red[tid >> 6] = best;
        __syncthreads();
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) best = red[w] > best ? red[w] : best;
    }
    if (tid < K) {
        const int32_t d = source == FQ_SPEC_LOOKUP ? fq_spec_lookup_draft(h, hn, best, gmin, tid + 1) : source == FQ_SPEC_GIVEN ? fq_spec_given_draft(q, nq, at, tid + 1) : -1;
        drafts[tid] = d;
        if (next_tok) next_tok[1 + tid] = d >= 0 ? d : 0;   // (a row without a draft is evaluated with a valid token and never accepted)
    }
}

// One workgroup = one sequence (sampler row blockIdx.x, the n_rows logits rows behind logits + blockIdx.x * n_rows * stride). Verify: sk_row on logits row
// 0, 1, ... with the ONE state of the sampler row, while fq_spec_go_on holds -- every draw goes through the row's window, generator, mu, stops, output slot and
// position exactly as a launch of k_sample_rows would have put it there. Then the history, the counters and the next pass's drafts.
// A row whose stops have ended it, or whose call has no draw left (st->left == 0), draws nothing and moves nothing: the pass was launched past the end.
template <bool EXT, bool TEXT>
__global__ void __launch_bounds__(FQ_SK_THREADS) k_verify_rows(const float * __restrict__ logits, int64_t stride, int n, int np,
        const fq_sample_row * __restrict__ rows, int32_t * __restrict__ ring, int ring_cap, int * __restrict__ head, uint32_t * __restrict__ mtg,
        uint64_t * __restrict__ sortg, int32_t * __restrict__ token, int * __restrict__ pos, int * __restrict__ steps, int32_t * __restrict__ out, int out_stride,
        const fq_stop_cfg * __restrict__ stop_cfg, fq_stop_state * __restrict__ stop_state, int * __restrict__ stop_skip,
        const fq_sample_ext * __restrict__ ext, float * __restrict__ mug, sk_text_args text, int ctx_limit, sk_spec_args sp) {
    __shared__ long long red_k[FQ_SK_THREADS / 64];
    const int row = blockIdx.x, tid = threadIdx.x;
    fq_spec_state * S = sp.st + row;
    int32_t * drafts = sp.drafts + row * FQ_SPEC_MAX_DRAFT;
    const int K = sp.n_rows - 1;
    // (every thread keeps the counters in registers: thread 0 alone writes them back, behind the barrier in front of the drafts)
    int left = S->left, hn = S->n_hist, at = S->given_at, nd = 0;
    const int nq = S->n_guess;
    bool ended = false;
    if (left != 0) {
        for (int j = 0;; ++j) {
            if (!sk_row<EXT, TEXT>(logits + ((int64_t) row * sp.n_rows + j) * stride, row, n, np, rows, ring, ring_cap, head, mtg, sortg, token, pos, steps, out, out_stride,
                                   stop_cfg, stop_state, stop_skip, ext, mug, text, ctx_limit, sp.draw + row)) { ended = true; break; }
            __syncthreads();                                // the draw, the row's state and its position are thread 0's (and the text wave's) writes
            const int32_t t = sp.draw[row];
            ended = stop_cfg && stop_cfg[row].on && fq_stop_finished(&stop_state[row]);
            nd = j + 1;
            if (left > 0) --left;
            ++at;
            if (sp.history && hn < sp.hist_cap) { if (tid == 0) sp.history[(int64_t) row * sp.hist_cap + hn] = t; ++hn; }
            // (the row moved to the position row j + 1 was evaluated at, unless it ended at the end of its cache -- then `ended` says so)
            if (!fq_spec_go_on(t, j < K ? drafts[j] : -1, ended, j, K, pos ? pos[row] : 0, pos ? sp.n_ctx : 0, left)) break;
        }
    } else if (stop_cfg && tid == 0) stop_skip[row] = 1;
    __syncthreads();                                        // (the history's new tokens; nobody reads this pass's drafts any more)
    if (sp.source != FQ_SPEC_OFF)
        sk_make_drafts(sp.source, sp.history + (int64_t) row * sp.hist_cap, hn, sp.ngram_min, sp.ngram_max, sp.guess, nq, at, K, drafts, sp.next_tok, red_k);
    if (tid == 0) {
        S->left = left; S->n_hist = hn; S->given_at = at; S->ended = ended ? 1 : 0;
        if (nd > 0) { S->passes += 1; S->draws += nd; S->hist[nd - 1] += 1; }
    }
}

// the drafts of a call's first pass, from the state as set_spec / the last call left it
__global__ void __launch_bounds__(FQ_SK_THREADS) k_spec_draft(sk_spec_args sp) {
    __shared__ long long red_k[FQ_SK_THREADS / 64];
    const fq_spec_state * S = sp.st;
    sk_make_drafts(sp.source, sp.history, S->n_hist, sp.ngram_min, sp.ngram_max, sp.guess, S->n_guess, S->given_at, sp.n_rows - 1, sp.drafts, sp.next_tok, red_k);
}
__global__ void __launch_bounds__(FQ_SK_THREADS) k_draft_lookup(const int32_t * __restrict__ h, int hn, int gmin, int gmax, int K, int32_t * __restrict__ drafts) {
    __shared__ long long red_k[FQ_SK_THREADS / 64];
    sk_make_drafts(FQ_SPEC_LOOKUP, h, hn, gmin, gmax, nullptr, 0, 0, K, drafts, nullptr, red_k);
}

static void spec_alloc(ggml_hip_sampler * s) {              // (outside any capture)
    if (s->spec_draw) return;
    HIP_CHECK(hipMalloc((void **) &s->spec_draw, 4));
    HIP_CHECK(hipMalloc((void **) &s->spec_state, sizeof(fq_spec_state)));
    HIP_CHECK(hipMalloc((void **) &s->spec_drafts, FQ_SPEC_MAX_DRAFT * 4));
}
void fq_sampler_spec_prepare(ggml_hip_sampler * s) { spec_alloc(s); }
static sk_spec_args spec_args(ggml_hip_sampler * s, const fq_spec_launch & sp) {
    return sk_spec_args{ sp.st, sp.history, sp.hist_cap, sp.guess, sp.drafts, sp.next_tok, s ? s->spec_draw : nullptr, sp.n_rows, sp.source, sp.ngram_min, sp.ngram_max, sp.n_ctx };
}
// the verify launch of ONE sequence (sampler row 0) in place of fq_launch_sample's: sp.n_rows logits rows, the row's state, position and output slot as there
void fq_launch_verify(ggml_hip_sampler * s, const fq_spec_launch & sp, const float * logits, int64_t row_stride, int32_t * token, int * pos, int * steps,
                      int32_t * out, hipStream_t st) {
    const bool ext = s->ext_rows > 0, txt = s->text_rows > 0;
    const sk_text_args text = txt ? sk_text_args{ s->text_cfg, s->text_state, s->vb_pool, s->vb_offs } : sk_text_args{ nullptr, nullptr, nullptr, nullptr };
    hipLaunchKernelGGL(txt ? (ext ? k_verify_rows<true, true> : k_verify_rows<false, true>) : (ext ? k_verify_rows<true, false> : k_verify_rows<false, false>),
                       dim3(1), dim3(FQ_SK_THREADS), 0, st, logits, row_stride,
                       s->n_vocab, s->np, s->rows, s->ring, s->n_ctx, s->head, s->mt, s->sort, token, pos, steps, out, 1,
                       s->stop_rows > 0 ? s->stop_cfg : nullptr, s->stop_rows > 0 ? s->stop_state : nullptr, s->stop_rows > 0 ? s->stop_skip : nullptr,
                       s->ext, s->mu, text, pos ? s->ctx_limit : 0, spec_args(s, sp));
}
void fq_launch_spec_draft(const fq_spec_launch & sp, hipStream_t st) {
    hipLaunchKernelGGL(k_spec_draft, dim3(1), dim3(FQ_SK_THREADS), 0, st, spec_args(nullptr, sp));
}

int fq_sampler_ctx_limit(const ggml_hip_sampler * s) { return s->ctx_limit; }
int fq_sampler_grammar_rows(const ggml_hip_sampler * s) { return s->gram_rows; }
int fq_sampler_guide_pairs(const ggml_hip_sampler * s) { return s->guide_pairs; }
const int * fq_sampler_lead_of(const ggml_hip_sampler * s) { return s->lead_host.data(); }
const int * fq_sampler_guide_of(const ggml_hip_sampler * s) { return s->guide_host.data(); }
int fq_sampler_drawing_stop_rows(const ggml_hip_sampler * s) {
    int n = 0;
    for (int r = 0; r < s->n_rows; ++r) n += s->stop_on[r] && s->lead_host[r] < 0;
    return n;
}
// the sampler part of a captured step's key: what fq_launch_sample / fq_launch_verify above choose by and hand the kernel, beyond what is fixed for the sampler's life
void fq_sampler_step_key(const ggml_hip_sampler * s, int64_t key[FQ_SAMPLER_KEY_WORDS]) {
    auto ptr = [](bool on, const void * p) { return on ? (int64_t)(uintptr_t) p : (int64_t) 0; };
    const bool stops = s->stop_rows > 0, txt = s->text_rows > 0;
    key[0] = ptr(stops, s->stop_cfg); key[1] = ptr(stops, s->stop_state); key[2] = ptr(stops, s->stop_skip);      // (0 while no row has stops: turning them on or off re-captures; a row's sequences and budget are device data)
    key[3] = s->ext_rows > 0;                               // (which instantiation of the kernel the step holds)
    key[4] = ptr(txt, s->text_cfg); key[5] = ptr(txt, s->text_state); key[6] = ptr(txt, s->vb_pool); key[7] = ptr(txt, s->vb_offs);      // (stop strings; 0 while no row has any -- the instantiation again)
    key[8] = s->ctx_limit;                                  // (the context stop: an argument of the launch, 0 while off)
    key[9] = ptr(s->gram_rows > 0, s->gram);                // (grammars: the rows' bindings, 0 while no row has one -- the instantiation again; a row's grammar and state are device data)
    key[10] = ptr(s->guide_pairs > 0, s->mixed);            // (guidance: 0 while no row has a guide row -- the mix launch and the guided kernel; pairs and scales are device data)
}
void fq_sampler_share_vocab_bytes(ggml_hip_sampler * s, uint8_t * pool, int32_t * offs) {
    if (s->vb_own) return;                                  // (its own arrays stay)
    s->vb_pool = pool; s->vb_offs = offs;
}
int * fq_sampler_steps(ggml_hip_sampler * s) { return s->steps; }
int32_t * fq_sampler_tokens(ggml_hip_sampler * s) { return s->tok; }
int fq_sampler_rows(const ggml_hip_sampler * s) { return s->n_rows; }
int fq_sampler_stop_rows(const ggml_hip_sampler * s) { return s->stop_rows; }
const fq_stop_cfg * fq_sampler_stop_cfg(const ggml_hip_sampler * s) { return s->stop_rows > 0 ? s->stop_cfg : nullptr; }
const fq_stop_state * fq_sampler_stop_state(const ggml_hip_sampler * s) { return s->stop_rows > 0 ? s->stop_state : nullptr; }
const int * fq_sampler_stop_skip(const ggml_hip_sampler * s) { return s->stop_rows > 0 ? s->stop_skip : nullptr; }

// the stop arrays, made by the first row that needs them: every row off, every state fresh
static void stops_alloc(ggml_hip_sampler * s, hipStream_t st) {
    if (s->stop_cfg) return;
    HIP_CHECK(hipMalloc((void **) &s->stop_cfg, sizeof(fq_stop_cfg) * s->n_rows));
    HIP_CHECK(hipMalloc((void **) &s->stop_state, sizeof(fq_stop_state) * s->n_rows));
    HIP_CHECK(hipMalloc((void **) &s->stop_skip, (size_t) s->n_rows * 4));
    std::vector<fq_stop_state> fresh(s->n_rows);
    for (auto & x : fresh) fq_stop_reset(&x);
    HIP_CHECK(hipMemsetAsync(s->stop_cfg, 0, sizeof(fq_stop_cfg) * s->n_rows, st));
    HIP_CHECK(hipMemsetAsync(s->stop_skip, 0, (size_t) s->n_rows * 4, st));
    HIP_CHECK(hipMemcpyAsync(s->stop_state, fresh.data(), sizeof(fq_stop_state) * s->n_rows, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));                    // (fresh is a local)
}
static void stops_mark(ggml_hip_sampler * s, int row, bool on) {
    s->stop_rows += (on ? 1 : 0) - (s->stop_on[row] ? 1 : 0);
    s->stop_on[row] = on ? 1 : 0;
}
// the text arrays, likewise: no row has strings, every ring fresh (fq_stopt_reset: all zero)
static void text_alloc(ggml_hip_sampler * s, hipStream_t st) {
    if (s->text_cfg) return;
    HIP_CHECK(hipMalloc((void **) &s->text_cfg, sizeof(fq_stopt_cfg) * s->n_rows));
    HIP_CHECK(hipMalloc((void **) &s->text_state, sizeof(fq_stopt_state) * s->n_rows));
    HIP_CHECK(hipMemsetAsync(s->text_cfg, 0, sizeof(fq_stopt_cfg) * s->n_rows, st));
    HIP_CHECK(hipMemsetAsync(s->text_state, 0, sizeof(fq_stopt_state) * s->n_rows, st));
}
static void text_mark(ggml_hip_sampler * s, int row, bool on) {
    s->text_rows += (on ? 1 : 0) - (s->text_on[row] ? 1 : 0);
    s->text_on[row] = on ? 1 : 0;
}
// a row's stops are on while either setter holds some for it: cfg.on (the struct's first word) follows the two host flags
static void stops_on_word(ggml_hip_sampler * s, int row, hipStream_t st) {
    const int32_t on = s->stop_ids[row] || s->text_on[row] || s->ctx_limit > 0;
    static_assert(offsetof(fq_stop_cfg, on) == 0, "cfg.on is written as the struct's first word");
    HIP_CHECK(hipMemcpyAsync(s->stop_cfg + row, &on, 4, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));                    // (on is a local)
    stops_mark(s, row, on != 0);
}

// the grammar bindings, likewise: no row has one (all zero: trans == nullptr)
static void gram_alloc(ggml_hip_sampler * s, hipStream_t st) {
    if (s->gram) return;
    HIP_CHECK(hipMalloc((void **) &s->gram, sizeof(fq_grammar_row) * s->n_rows));
    HIP_CHECK(hipMemsetAsync(s->gram, 0, sizeof(fq_grammar_row) * s->n_rows, st));
}
static void gram_mark(ggml_hip_sampler * s, int row, ggml_hip_grammar * g) {
    if (g) fq_grammar_bind(g, 1);                           // (first: g may be the grammar the row holds already)
    if (s->gram_host[row]) fq_grammar_bind(s->gram_host[row], -1);
    s->gram_rows += (g ? 1 : 0) - (s->gram_host[row] ? 1 : 0);
    s->gram_host[row] = g;
}

// the vocabulary's bytes as device arrays (ggml_hip_sampler_set_vocab_bytes, falcon_hip_model_set_vocab): 0, or 1 after a message with nothing made
int fq_vocab_bytes_upload(const char * who, const uint8_t * pool, const int32_t * offs, int n_vocab, uint8_t ** pool_dev, int32_t ** offs_dev) {
    if (!offs || offs[0] != 0) { fprintf(stderr, "%s: the offsets do not start at 0\n", who); return 1; }
    for (int t = 0; t < n_vocab; ++t) if (offs[t + 1] < offs[t]) { fprintf(stderr, "%s: the offsets do not ascend at token %d (%d after %d)\n", who, t, offs[t + 1], offs[t]); return 1; }
    const int64_t bytes = offs[n_vocab];
    if (bytes > FQ_SK_MAX_VOCAB_BYTES) { fprintf(stderr, "%s: a byte pool of %lld bytes (at most %d)\n", who, (long long) bytes, FQ_SK_MAX_VOCAB_BYTES); return 1; }
    if (bytes > 0 && !pool) { fprintf(stderr, "%s: no byte pool\n", who); return 1; }
    hipStream_t st = fq_ctx().stream;
    HIP_CHECK(hipMalloc((void **) pool_dev, (size_t)(bytes > 0 ? bytes : 1)));
    HIP_CHECK(hipMalloc((void **) offs_dev, ((size_t) n_vocab + 1) * 4));
    if (bytes > 0) HIP_CHECK(hipMemcpyAsync(*pool_dev, pool, (size_t) bytes, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(*offs_dev, offs, ((size_t) n_vocab + 1) * 4, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}

// ------------------------------------------------------------------------------------------------ C ABI (include/ggml-hip-ops.h)
extern "C" ggml_hip_sampler * ggml_hip_sampler_create(int n_rows, int n_vocab, int n_ctx) {
    if (n_rows < 1 || n_vocab < 1 || n_vocab > FQ_SK_MAX_VOCAB || n_ctx < 1) {
        fprintf(stderr, "ggml-hip: sampler_create(%d rows, n_vocab %d, n_ctx %d): needs n_rows >= 1, 1 <= n_vocab <= %d, n_ctx >= 1\n", n_rows, n_vocab, n_ctx, FQ_SK_MAX_VOCAB);
        return nullptr;
    }
    hipStream_t st = fq_ctx().stream;
    ggml_hip_sampler * s = new ggml_hip_sampler();
    s->n_rows = n_rows; s->n_vocab = n_vocab; s->n_ctx = n_ctx;
    s->np = 1;
    while (s->np < n_vocab) s->np <<= 1;
    s->W.assign(n_rows, 0);
    s->stop_on.assign(n_rows, 0);
    s->stop_ids.assign(n_rows, 0);
    s->text_on.assign(n_rows, 0);
    s->gram_host.assign(n_rows, nullptr);
    s->guide_host.assign(n_rows, -1);
    s->lead_host.assign(n_rows, -1);
    s->scale_host.assign(n_rows, 1.0f);
    s->ext_host.assign(n_rows, fq_sample_ext{ 1.0f, 1.0f, 0.0f, 0.0f, 0 });
    HIP_CHECK(hipMalloc((void **) &s->ext, sizeof(fq_sample_ext) * n_rows));
    HIP_CHECK(hipMalloc((void **) &s->mu, (size_t) n_rows * 4));
    HIP_CHECK(hipMalloc((void **) &s->rows, sizeof(fq_sample_row) * n_rows));
    HIP_CHECK(hipMalloc((void **) &s->ring, (size_t) n_rows * n_ctx * 4));
    HIP_CHECK(hipMalloc((void **) &s->head, (size_t) n_rows * 4));
    HIP_CHECK(hipMalloc((void **) &s->mt, (size_t) n_rows * (FQ_MT_N + 1) * 4));
    HIP_CHECK(hipMalloc((void **) &s->sort, (size_t) n_rows * s->np * 8));
    HIP_CHECK(hipMalloc((void **) &s->steps, (size_t) n_rows * 4));
    HIP_CHECK(hipMalloc((void **) &s->tok, (size_t) n_rows * 4));
    // every row greedy, no penalties, empty window, generator seeded with 0, until ggml_hip_sampler_set_row
    std::vector<fq_sample_row> r(n_rows);
    for (auto & x : r) { memset(&x, 0, sizeof x); x.penalty = 1.0f; x.top_p = 1.0f; }
    std::vector<uint32_t> mt((size_t) n_rows * (FQ_MT_N + 1));
    for (int i = 0; i < n_rows; ++i) { int mti; fq_mt_seed(&mt[(size_t) i * (FQ_MT_N + 1)], &mti, 0); mt[(size_t) i * (FQ_MT_N + 1) + FQ_MT_N] = (uint32_t) mti; }
    HIP_CHECK(hipMemcpyAsync(s->rows, r.data(), sizeof(fq_sample_row) * n_rows, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(s->mt, mt.data(), mt.size() * 4, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(s->ext, s->ext_host.data(), sizeof(fq_sample_ext) * n_rows, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemsetAsync(s->mu, 0, (size_t) n_rows * 4, st));
    HIP_CHECK(hipMemsetAsync(s->head, 0, (size_t) n_rows * 4, st));
    HIP_CHECK(hipMemsetAsync(s->steps, 0, (size_t) n_rows * 4, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return s;
}

extern "C" void ggml_hip_sampler_free(ggml_hip_sampler * s) {
    if (!s) return;
    HIP_CHECK(hipStreamSynchronize(fq_ctx().stream));
    for (void * p : { (void *) s->rows, (void *) s->ring, (void *) s->head, (void *) s->mt, (void *) s->sort, (void *) s->steps, (void *) s->tok, (void *) s->ext, (void *) s->mu }) HIP_CHECK(hipFree(p));
    for (void * p : { (void *) s->stop_cfg, (void *) s->stop_state, (void *) s->stop_skip, (void *) s->text_cfg, (void *) s->text_state }) if (p) HIP_CHECK(hipFree(p));
    if (s->vb_own) { HIP_CHECK(hipFree(s->vb_pool)); HIP_CHECK(hipFree(s->vb_offs)); }
    for (void * p : { (void *) s->spec_draw, (void *) s->spec_state, (void *) s->spec_drafts, (void *) s->gram }) if (p) HIP_CHECK(hipFree(p));
    for (void * p : { (void *) s->guide_of, (void *) s->lead_of, (void *) s->mix_lead, (void *) s->guide_scale, (void *) s->mixed }) if (p) HIP_CHECK(hipFree(p));
    for (ggml_hip_grammar * g : s->gram_host) if (g) fq_grammar_bind(g, -1);
    delete s;
}

// set_row and set_row_ext behind their own refusals: the checks both share, then the row's parameters, window, generator, stages (x) and mu
static int set_row_checked(ggml_hip_sampler * s, int row, const ggml_hip_sampling * p, const int32_t * history, int n_history, const fq_sample_ext & x) {
    if (p->n_bias < 0 || p->n_bias > FQ_SAMPLE_MAX_BIAS) { fprintf(stderr, "ggml-hip: sampler_set_row: %d logit biases (at most %d)\n", p->n_bias, FQ_SAMPLE_MAX_BIAS); return 1; }
    for (int i = 0; i < p->n_bias; ++i) {
        if (p->bias_id[i] < 0 || p->bias_id[i] >= s->n_vocab) { fprintf(stderr, "ggml-hip: sampler_set_row: logit bias id %d is outside [0, %d)\n", p->bias_id[i], s->n_vocab); return 1; }
        for (int j = 0; j < i; ++j) if (p->bias_id[j] == p->bias_id[i]) { fprintf(stderr, "ggml-hip: sampler_set_row: logit bias id %d given twice\n", p->bias_id[i]); return 1; }
    }
    for (int i = 0; i < n_history; ++i) if (history[i] < 0 || history[i] >= s->n_vocab) { fprintf(stderr, "ggml-hip: sampler_set_row: history token %d is outside [0, %d)\n", history[i], s->n_vocab); return 1; }
    // falcon_main.cpp:862, 949: the last min(repeat_last_n, n_ctx) entries (-1: n_ctx) of a window of n_ctx tokens that starts as zeros
    const int W = p->repeat_last_n < 0 || p->repeat_last_n > s->n_ctx ? s->n_ctx : p->repeat_last_n;
    if (W > FQ_SK_MAX_WINDOW) { fprintf(stderr, "ggml-hip: sampler_set_row: a window of %d tokens (at most %d)\n", W, FQ_SK_MAX_WINDOW); return 1; }
    fq_sample_row r;
    memset(&r, 0, sizeof r);
    r.temp = p->temp; r.top_p = p->top_p; r.penalty = p->repeat_penalty; r.alpha_f = p->alpha_frequency; r.alpha_p = p->alpha_presence;
    r.top_k = p->top_k; r.W = W; r.n_bias = p->n_bias;
    for (int i = 0; i < p->n_bias; ++i) { r.bias_id[i] = p->bias_id[i]; r.bias[i] = p->bias[i]; }
    std::vector<int32_t> win((size_t) W + 1, 0);
    for (int j = 0; j < W; ++j) { const int h = n_history - W + j; win[j] = h >= 0 ? history[h] : 0; }
    std::vector<uint32_t> mt(FQ_MT_N + 1);
    int mti;
    fq_mt_seed(mt.data(), &mti, p->seed);
    mt[FQ_MT_N] = (uint32_t) mti;
    const int zero = 0;
    hipStream_t st = fq_ctx().stream;
    HIP_CHECK(hipMemcpyAsync(s->rows + row, &r, sizeof r, hipMemcpyHostToDevice, st));
    if (W > 0) HIP_CHECK(hipMemcpyAsync(s->ring + (int64_t) row * s->n_ctx, win.data(), (size_t) W * 4, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(s->head + row, &zero, 4, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(s->mt + (int64_t) row * (FQ_MT_N + 1), mt.data(), mt.size() * 4, hipMemcpyHostToDevice, st));
    const float mu0 = 2.0f * x.tau;                         // falcon_main.cpp:965, 970: static float mirostat_mu = 2.0f * mirostat_tau
    HIP_CHECK(hipMemcpyAsync(s->ext + row, &x, sizeof x, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(s->mu + row, &mu0, 4, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));
    s->W[row] = W;
    s->ext_rows += (ext_uses(x) ? 1 : 0) - (ext_uses(s->ext_host[row]) ? 1 : 0);
    s->ext_host[row] = x;
    return 0;
}

extern "C" int ggml_hip_sampler_set_row(ggml_hip_sampler * s, int row, const ggml_hip_sampling * p, const int32_t * history, int n_history) {
    if (!s || !p || row < 0 || row >= s->n_rows || n_history < 0 || (n_history > 0 && !history)) { fprintf(stderr, "ggml-hip: sampler_set_row: bad row %d or arguments\n", row); return 1; }
    if (p->tfs_z != 1.0f || p->typical_p != 1.0f || p->mirostat != 0) {
        fprintf(stderr, "ggml-hip: sampler_set_row: tail-free (tfs_z %g), typical (typical_p %g) and mirostat (%d) sampling are not supported\n", p->tfs_z, p->typical_p, p->mirostat);
        return 1;
    }
    return set_row_checked(s, row, p, history, n_history, fq_sample_ext{ 1.0f, 1.0f, 0.0f, 0.0f, 0 });
}

extern "C" int ggml_hip_sampler_set_row_ext(ggml_hip_sampler * s, int row, const ggml_hip_sampling_ext * px, const int32_t * history, int n_history) {
    if (!s || !px || row < 0 || row >= s->n_rows || n_history < 0 || (n_history > 0 && !history)) { fprintf(stderr, "ggml-hip: sampler_set_row_ext: bad row %d or arguments\n", row); return 1; }
    const ggml_hip_sampling * p = &px->base;
    if (p->mirostat < 0 || p->mirostat > 2) { fprintf(stderr, "ggml-hip: sampler_set_row_ext: mirostat %d (0, 1 or 2)\n", p->mirostat); return 1; }
    if (!isfinite(px->mirostat_tau) || !isfinite(px->mirostat_eta)) { fprintf(stderr, "ggml-hip: sampler_set_row_ext: mirostat tau %g or eta %g is not finite\n", px->mirostat_tau, px->mirostat_eta); return 1; }
    const fq_sample_ext x = { p->tfs_z, p->typical_p, px->mirostat_tau, px->mirostat_eta, p->mirostat };
    // tail-free and typical run on the LDS form's survivors (mirostat and greedy ignore both stages)
    if ((!(x.tfs_z >= 1.0f) || !(x.typical_p >= 1.0f)) && x.mirostat == 0 && p->temp > 0.0f && (p->top_k < 1 || p->top_k > FQ_SK_SMALL_K)) {
        fprintf(stderr, "ggml-hip: sampler_set_row_ext: tail-free (tfs_z %g) and typical (typical_p %g) need 1 <= top_k <= %d (top_k %d)\n", x.tfs_z, x.typical_p, FQ_SK_SMALL_K, p->top_k);
        return 1;
    }
    return set_row_checked(s, row, p, history, n_history, x);
}

extern "C" int ggml_hip_sampler_get_mu(ggml_hip_sampler * s, float * mu_out) {
    if (!s || !mu_out) return 1;
    hipStream_t st = fq_ctx().stream;
    HIP_CHECK(hipMemcpyAsync(mu_out, s->mu, (size_t) s->n_rows * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}

// a row's generator as std::mt19937 holds it: 624 state words and the position (624 right after seeding). Nothing else of the row moves.
extern "C" int ggml_hip_sampler_get_rng(ggml_hip_sampler * s, int row, uint32_t * words_out, int32_t * pos_out) {
    if (!s || row < 0 || row >= s->n_rows || !words_out || !pos_out) { fprintf(stderr, "ggml-hip: sampler_get_rng: bad row %d or arguments\n", row); return 1; }
    uint32_t mt[FQ_MT_N + 1];
    hipStream_t st = fq_ctx().stream;
    HIP_CHECK(hipMemcpyAsync(mt, s->mt + (int64_t) row * (FQ_MT_N + 1), sizeof mt, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    memcpy(words_out, mt, FQ_MT_N * 4);
    *pos_out = (int32_t) mt[FQ_MT_N];
    return 0;
}
extern "C" int ggml_hip_sampler_set_rng(ggml_hip_sampler * s, int row, const uint32_t * words, int32_t pos) {
    if (!s || row < 0 || row >= s->n_rows || !words || pos < 0 || pos > FQ_MT_N) { fprintf(stderr, "ggml-hip: sampler_set_rng: bad row %d, position %d or arguments\n", row, pos); return 1; }
    uint32_t mt[FQ_MT_N + 1];
    memcpy(mt, words, FQ_MT_N * 4);
    mt[FQ_MT_N] = (uint32_t) pos;
    hipStream_t st = fq_ctx().stream;
    HIP_CHECK(hipMemcpyAsync(s->mt + (int64_t) row * (FQ_MT_N + 1), mt, sizeof mt, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}

extern "C" int ggml_hip_sampler_copy_row(ggml_hip_sampler * dst, int dst_row, const ggml_hip_sampler * src, int src_row) {
    if (!dst || !src || dst_row < 0 || dst_row >= dst->n_rows || src_row < 0 || src_row >= src->n_rows || dst->n_vocab != src->n_vocab) {
        fprintf(stderr, "ggml-hip: sampler_copy_row: bad rows (%d -> %d) or different vocabularies\n", src_row, dst_row);
        return 1;
    }
    const int W = src->W[src_row];
    if (W > dst->n_ctx) { fprintf(stderr, "ggml-hip: sampler_copy_row: a window of %d tokens does not fit n_ctx %d\n", W, dst->n_ctx); return 1; }
    if (src->text_on[src_row] && !dst->vb_pool) { fprintf(stderr, "ggml-hip: sampler_copy_row: row %d has stop strings and the destination has no vocabulary bytes\n", src_row); return 1; }
    if (dst == src && dst_row == src_row) return 0;
    hipStream_t st = fq_ctx().stream;
    HIP_CHECK(hipMemcpyAsync(dst->rows + dst_row, src->rows + src_row, sizeof(fq_sample_row), hipMemcpyDeviceToDevice, st));
    if (W > 0) HIP_CHECK(hipMemcpyAsync(dst->ring + (int64_t) dst_row * dst->n_ctx, src->ring + (int64_t) src_row * src->n_ctx, (size_t) W * 4, hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipMemcpyAsync(dst->head + dst_row, src->head + src_row, 4, hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipMemcpyAsync(dst->mt + (int64_t) dst_row * (FQ_MT_N + 1), src->mt + (int64_t) src_row * (FQ_MT_N + 1), (FQ_MT_N + 1) * 4, hipMemcpyDeviceToDevice, st));
    dst->W[dst_row] = W;
    HIP_CHECK(hipMemcpyAsync(dst->ext + dst_row, src->ext + src_row, sizeof(fq_sample_ext), hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipMemcpyAsync(dst->mu + dst_row, src->mu + src_row, 4, hipMemcpyDeviceToDevice, st));
    dst->ext_rows += (ext_uses(src->ext_host[src_row]) ? 1 : 0) - (ext_uses(dst->ext_host[dst_row]) ? 1 : 0);
    dst->ext_host[dst_row] = src->ext_host[src_row];
    // the row's stops and their state travel with it; a sampler that never held stops gets the arrays only for a row that has some
    const bool on = src->stop_on[src_row];
    if (on) stops_alloc(dst, st);
    if (dst->stop_cfg) {
        if (on) {
            HIP_CHECK(hipMemcpyAsync(dst->stop_cfg + dst_row, src->stop_cfg + src_row, sizeof(fq_stop_cfg), hipMemcpyDeviceToDevice, st));
            HIP_CHECK(hipMemcpyAsync(dst->stop_state + dst_row, src->stop_state + src_row, sizeof(fq_stop_state), hipMemcpyDeviceToDevice, st));
        } else if (dst->stop_on[dst_row]) {
            fq_stop_state fresh;
            fq_stop_reset(&fresh);
            HIP_CHECK(hipMemsetAsync(dst->stop_cfg + dst_row, 0, sizeof(fq_stop_cfg), st));
            HIP_CHECK(hipMemcpyAsync(dst->stop_state + dst_row, &fresh, sizeof fresh, hipMemcpyHostToDevice, st));
            HIP_CHECK(hipStreamSynchronize(st));            // (fresh is a local)
        }
        stops_mark(dst, dst_row, on);
        dst->stop_ids[dst_row] = src->stop_ids[src_row];
    }
    // ... and its stop strings, ring and cut_bytes
    const bool txt = src->text_on[src_row];
    if (txt) text_alloc(dst, st);
    if (dst->text_cfg) {
        if (txt) {
            HIP_CHECK(hipMemcpyAsync(dst->text_cfg + dst_row, src->text_cfg + src_row, sizeof(fq_stopt_cfg), hipMemcpyDeviceToDevice, st));
            HIP_CHECK(hipMemcpyAsync(dst->text_state + dst_row, src->text_state + src_row, sizeof(fq_stopt_state), hipMemcpyDeviceToDevice, st));
        } else if (dst->text_on[dst_row]) {
            HIP_CHECK(hipMemsetAsync(dst->text_cfg + dst_row, 0, sizeof(fq_stopt_cfg), st));
            HIP_CHECK(hipMemsetAsync(dst->text_state + dst_row, 0, sizeof(fq_stopt_state), st));
        }
        text_mark(dst, dst_row, txt);
    }
    // (the word a context stop keeps on is the destination's own, not the source's)
    if (dst->stop_cfg && (dst->ctx_limit > 0) != (src->ctx_limit > 0)) stops_on_word(dst, dst_row, st);
    // ... and its grammar and state (the descriptor holds both)
    ggml_hip_grammar * g = src->gram_host[src_row];
    if (g) gram_alloc(dst, st);
    if (dst->gram) {
        if (g) HIP_CHECK(hipMemcpyAsync(dst->gram + dst_row, src->gram + src_row, sizeof(fq_grammar_row), hipMemcpyDeviceToDevice, st));
        else if (dst->gram_host[dst_row]) HIP_CHECK(hipMemsetAsync(dst->gram + dst_row, 0, sizeof(fq_grammar_row), st));
        gram_mark(dst, dst_row, g);
    }
    return 0;
}

extern "C" int ggml_hip_sampler_set_stops(ggml_hip_sampler * s, int row, const ggml_hip_stops * stops) {
    if (!s || row < 0 || row >= s->n_rows) { fprintf(stderr, "ggml-hip: sampler_set_stops: bad row %d\n", row); return 1; }
    fq_stop_cfg c;
    memset(&c, 0, sizeof c);
    if (stops) {
        if (stops->n_seqs < 0 || stops->n_seqs > FQ_STOP_MAX_SEQS) { fprintf(stderr, "ggml-hip: sampler_set_stops: %d stop sequences (0..%d)\n", stops->n_seqs, FQ_STOP_MAX_SEQS); return 1; }
        if (stops->max_tokens < 0) { fprintf(stderr, "ggml-hip: sampler_set_stops: max_tokens %d < 0\n", stops->max_tokens); return 1; }
        for (int k = 0; k < stops->n_seqs; ++k) {
            if (stops->len[k] < 1 || stops->len[k] > FQ_STOP_MAX_LEN) { fprintf(stderr, "ggml-hip: sampler_set_stops: stop sequence %d has %d tokens (1..%d)\n", k, stops->len[k], FQ_STOP_MAX_LEN); return 1; }
            for (int j = 0; j < stops->len[k]; ++j)
                if (stops->tok[k][j] < 0 || stops->tok[k][j] >= s->n_vocab) { fprintf(stderr, "ggml-hip: sampler_set_stops: token %d of stop sequence %d is outside [0, %d)\n", stops->tok[k][j], k, s->n_vocab); return 1; }
        }
        c.n_seqs = stops->n_seqs; c.max_tokens = stops->max_tokens;
        for (int k = 0; k < stops->n_seqs; ++k) { c.len[k] = stops->len[k]; for (int j = 0; j < stops->len[k]; ++j) c.tok[k][j] = stops->tok[k][j]; }
    }
    if (!stops && !s->stop_cfg) return 0;                   // (never on: nothing to turn off)
    hipStream_t st = fq_ctx().stream;
    stops_alloc(s, st);
    fq_stop_state fresh;
    fq_stop_reset(&fresh);
    c.on = stops != nullptr || s->text_on[row] || s->ctx_limit > 0;      // (a row with stop strings, or under a context stop, stays on without id sequences or a budget)
    HIP_CHECK(hipMemcpyAsync(s->stop_cfg + row, &c, sizeof c, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(s->stop_state + row, &fresh, sizeof fresh, hipMemcpyHostToDevice, st));
    if (s->text_on[row]) HIP_CHECK(hipMemsetAsync(s->text_state + row, 0, sizeof(fq_stopt_state), st));      // the shared state starts afresh: ring and cut_bytes too
    HIP_CHECK(hipStreamSynchronize(st));
    s->stop_ids[row] = stops != nullptr;
    stops_mark(s, row, c.on != 0);
    return 0;
}

// ---- the end of the cache (fq_stop.h: fq_stop_context, fq_stop_resume)
extern "C" int ggml_hip_sampler_set_context_stop(ggml_hip_sampler * s, int limit) {
    if (!s || limit < 0) { fprintf(stderr, "ggml-hip: sampler_set_context_stop: limit %d < 0\n", limit); return 1; }
    if (limit > 0 && s->guide_pairs > 0) { fprintf(stderr, "ggml-hip: sampler_set_context_stop: %d rows have guide rows (ggml_hip_sampler_set_guidance), which end with their leaders only: take them off first\n", s->guide_pairs); return 1; }
    if ((limit > 0) == (s->ctx_limit > 0)) { s->ctx_limit = limit; return 0; }
    if (limit == 0 && !s->stop_cfg) return 0;               // (never on: nothing to turn off)
    hipStream_t st = fq_ctx().stream;
    stops_alloc(s, st);
    s->ctx_limit = limit;
    for (int row = 0; row < s->n_rows; ++row) stops_on_word(s, row, st);      // (a row that was off has a fresh state: stops_alloc, set_stops(NULL) and set_stop_text(NULL) leave one)
    return 0;
}
extern "C" int ggml_hip_sampler_resume(ggml_hip_sampler * s, int row) {
    if (!s || row < 0 || row >= s->n_rows) { fprintf(stderr, "ggml-hip: sampler_resume: bad row %d\n", row); return 1; }
    fq_stop_state h;
    fq_stop_reset(&h);
    hipStream_t st = fq_ctx().stream;
    if (s->stop_state && s->stop_on[row]) {
        HIP_CHECK(hipMemcpyAsync(&h, s->stop_state + row, sizeof h, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
    }
    if (!fq_stop_resume(&h)) { fprintf(stderr, "ggml-hip: sampler_resume: row %d did not end at the end of its cache (reason %d)\n", row, h.reason); return 1; }
    static_assert(offsetof(fq_stop_state, reason) == 4, "the reason is written as the state's second word");
    HIP_CHECK(hipMemcpyAsync(&s->stop_state[row].reason, &h.reason, 4, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));                    // (h is a local)
    return 0;
}

// ---- stop strings (fq_stop_text.h)
extern "C" int ggml_hip_sampler_set_vocab_bytes(ggml_hip_sampler * s, const uint8_t * pool_host, const int32_t * offsets_host) {
    if (!s) return 1;
    uint8_t * pool = nullptr; int32_t * offs = nullptr;
    if (fq_vocab_bytes_upload("ggml-hip: sampler_set_vocab_bytes", pool_host, offsets_host, s->n_vocab, &pool, &offs)) return 1;
    HIP_CHECK(hipStreamSynchronize(fq_ctx().stream));       // (a launch in flight may read the arrays this replaces)
    if (s->vb_own) { HIP_CHECK(hipFree(s->vb_pool)); HIP_CHECK(hipFree(s->vb_offs)); }
    s->vb_pool = pool; s->vb_offs = offs; s->vb_own = true;
    return 0;
}

extern "C" int ggml_hip_sampler_set_stop_text(ggml_hip_sampler * s, int row, const ggml_hip_stop_text * text) {
    if (!s || row < 0 || row >= s->n_rows) { fprintf(stderr, "ggml-hip: sampler_set_stop_text: bad row %d\n", row); return 1; }
    fq_stopt_cfg c;
    memset(&c, 0, sizeof c);
    if (text) {
        if (text->n < 0 || text->n > FQ_STOPT_MAX) { fprintf(stderr, "ggml-hip: sampler_set_stop_text: %d stop strings (0..%d)\n", text->n, FQ_STOPT_MAX); return 1; }
        for (int k = 0; k < text->n; ++k)
            if (text->len[k] < 1 || text->len[k] > FQ_STOPT_MAX_LEN) { fprintf(stderr, "ggml-hip: sampler_set_stop_text: stop string %d has %d bytes (1..%d)\n", k, text->len[k], FQ_STOPT_MAX_LEN); return 1; }
        if (!s->vb_pool) { fprintf(stderr, "ggml-hip: sampler_set_stop_text: no vocabulary bytes set (ggml_hip_sampler_set_vocab_bytes)\n"); return 1; }
        c.n = text->n;
        for (int k = 0; k < text->n; ++k) { c.len[k] = text->len[k]; memcpy(c.bytes[k], text->bytes[k], (size_t) text->len[k]); }
    }
    if (!text && !s->text_cfg) return 0;                    // (never on: nothing to turn off)
    hipStream_t st = fq_ctx().stream;
    stops_alloc(s, st);
    text_alloc(s, st);
    fq_stop_state fresh;
    fq_stop_reset(&fresh);
    HIP_CHECK(hipMemcpyAsync(s->text_cfg + row, &c, sizeof c, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemsetAsync(s->text_state + row, 0, sizeof(fq_stopt_state), st));
    HIP_CHECK(hipMemcpyAsync(s->stop_state + row, &fresh, sizeof fresh, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));                    // (c and fresh are locals)
    text_mark(s, row, text != nullptr);
    stops_on_word(s, row, st);
    return 0;
}

extern "C" int ggml_hip_sampler_get_stop_text(ggml_hip_sampler * s, int32_t * cut_bytes_out) {
    if (!s || !cut_bytes_out) return 1;
    hipStream_t st = fq_ctx().stream;
    std::vector<fq_stopt_state> h(s->n_rows);
    for (auto & x : h) fq_stopt_reset(&x);
    if (s->text_state) HIP_CHECK(hipMemcpyAsync(h.data(), s->text_state, sizeof(fq_stopt_state) * s->n_rows, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    for (int r = 0; r < s->n_rows; ++r) cut_bytes_out[r] = s->text_on[r] ? h[r].cut_bytes : 0;
    return 0;
}

extern "C" int ggml_hip_sampler_get_stops(ggml_hip_sampler * s, int32_t * n_drawn_out, int32_t * reason_out) {
    if (!s) return 1;
    hipStream_t st = fq_ctx().stream;
    std::vector<fq_stop_state> h(s->n_rows);
    for (auto & x : h) fq_stop_reset(&x);
    if (s->stop_state) HIP_CHECK(hipMemcpyAsync(h.data(), s->stop_state, sizeof(fq_stop_state) * s->n_rows, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    for (int r = 0; r < s->n_rows; ++r) {
        if (n_drawn_out) n_drawn_out[r] = s->stop_on[r] ? h[r].n_drawn : 0;
        if (reason_out) reason_out[r] = s->stop_on[r] ? h[r].reason : FQ_STOP_RUNNING;
    }
    return 0;
}

// ---- grammars (fq_grammar.h, kernels_grammar.hip)
extern "C" int ggml_hip_sampler_set_grammar(ggml_hip_sampler * s, int row, ggml_hip_grammar * g, int state) {
    if (!s || row < 0 || row >= s->n_rows) { fprintf(stderr, "ggml-hip: sampler_set_grammar: bad row %d\n", row); return 1; }
    fq_grammar_row d;
    memset(&d, 0, sizeof d);
    if (g) {
        if (fq_grammar_vocab(g) != s->n_vocab) { fprintf(stderr, "ggml-hip: sampler_set_grammar: a grammar over %d tokens for a sampler with n_vocab %d\n", fq_grammar_vocab(g), s->n_vocab); return 1; }
        if (fq_grammar_row_of(g, state, &d)) { fprintf(stderr, "ggml-hip: sampler_set_grammar: state %d is outside the automaton (-1: its start state)\n", state); return 1; }
    }
    if (!g && !s->gram) return 0;                           // (never on: nothing to turn off)
    hipStream_t st = fq_ctx().stream;
    gram_alloc(s, st);
    HIP_CHECK(hipMemcpyAsync(s->gram + row, &d, sizeof d, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));                    // (d is a local)
    gram_mark(s, row, g);
    return 0;
}
extern "C" int ggml_hip_sampler_get_grammar_state(ggml_hip_sampler * s, int32_t * states_out) {
    if (!s || !states_out) return 1;
    hipStream_t st = fq_ctx().stream;
    std::vector<fq_grammar_row> h(s->n_rows);
    if (s->gram) HIP_CHECK(hipMemcpyAsync(h.data(), s->gram, sizeof(fq_grammar_row) * s->n_rows, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    for (int r = 0; r < s->n_rows; ++r) states_out[r] = s->gram_host[r] ? h[r].state : -1;
    return 0;
}

// ---- guidance (fq_guide.h, kernels_guide.hip)
// the pair arrays, made by the first pair: no row leads or guides (outside any capture)
static void guide_alloc(ggml_hip_sampler * s, hipStream_t st) {
    if (s->mixed) return;
    s->mixed_stride = ((int64_t) s->n_vocab + 3) & ~(int64_t) 3;
    HIP_CHECK(hipMalloc((void **) &s->guide_of, (size_t) s->n_rows * 4));
    HIP_CHECK(hipMalloc((void **) &s->lead_of, (size_t) s->n_rows * 4));
    HIP_CHECK(hipMalloc((void **) &s->mix_lead, (size_t) s->n_rows * 4));
    HIP_CHECK(hipMalloc((void **) &s->guide_scale, (size_t) s->n_rows * 4));
    HIP_CHECK(hipMalloc((void **) &s->mixed, (size_t) s->n_rows * s->mixed_stride * 4));
    HIP_CHECK(hipMemsetAsync(s->guide_of, 0xff, (size_t) s->n_rows * 4, st));
    HIP_CHECK(hipMemsetAsync(s->lead_of, 0xff, (size_t) s->n_rows * 4, st));
    HIP_CHECK(hipMemsetAsync(s->mix_lead, 0xff, (size_t) s->n_rows * 4, st));
    HIP_CHECK(hipMemsetAsync(s->guide_scale, 0, (size_t) s->n_rows * 4, st));
}
// row's words of the three index arrays and its scale, from the host copies
static void guide_upload(ggml_hip_sampler * s, int row, hipStream_t st) {
    const int32_t w[3] = { s->guide_host[row], s->lead_host[row], s->guide_host[row] >= 0 ? row : -1 };
    HIP_CHECK(hipMemcpyAsync(s->guide_of + row, &w[0], 4, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(s->lead_of + row, &w[1], 4, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(s->mix_lead + row, &w[2], 4, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(s->guide_scale + row, &s->scale_host[row], 4, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));                    // (w is a local)
}

extern "C" int ggml_hip_sampler_set_guidance(ggml_hip_sampler * s, int row, int guide_row, float scale) {
    if (!s || row < 0 || row >= s->n_rows || guide_row < -1 || guide_row >= s->n_rows) { fprintf(stderr, "ggml-hip: sampler_set_guidance: row %d or guide row %d is out of range\n", row, guide_row); return 1; }
    hipStream_t st = fq_ctx().stream;
    if (guide_row < 0) {                                    // off for the row
        const int old = s->guide_host[row];
        if (old < 0) return 0;                              // (never on: nothing to turn off)
        s->guide_host[row] = -1; s->lead_host[old] = -1; s->scale_host[row] = 1.0f;
        s->guide_pairs -= 1;
        guide_upload(s, row, st);
        guide_upload(s, old, st);
        return 0;
    }
    if (row == guide_row) { fprintf(stderr, "ggml-hip: sampler_set_guidance: row %d cannot guide itself\n", row); return 1; }
    if (!isfinite(scale)) { fprintf(stderr, "ggml-hip: sampler_set_guidance: scale %g is not finite\n", scale); return 1; }
    if (s->lead_host[row] >= 0) { fprintf(stderr, "ggml-hip: sampler_set_guidance: row %d is the guide row of row %d\n", row, s->lead_host[row]); return 1; }
    if (s->guide_host[guide_row] >= 0) { fprintf(stderr, "ggml-hip: sampler_set_guidance: guide row %d leads row %d\n", guide_row, s->guide_host[guide_row]); return 1; }
    if (s->lead_host[guide_row] >= 0 && s->lead_host[guide_row] != row) { fprintf(stderr, "ggml-hip: sampler_set_guidance: guide row %d guides row %d already\n", guide_row, s->lead_host[guide_row]); return 1; }
    if (s->ctx_limit > 0) { fprintf(stderr, "ggml-hip: sampler_set_guidance: the context stop is on (ggml_hip_sampler_set_context_stop) and a guide row ends with its leader only: turn it off first\n"); return 1; }
    guide_alloc(s, st);
    const int old = s->guide_host[row];
    if (old >= 0 && old != guide_row) { s->lead_host[old] = -1; guide_upload(s, old, st); }
    if (old < 0) s->guide_pairs += 1;
    s->guide_host[row] = guide_row; s->lead_host[guide_row] = row; s->scale_host[row] = scale;
    guide_upload(s, guide_row, st);                         // (the guide row leaves the launch before the leader reads from a mixed row)
    guide_upload(s, row, st);
    return 0;
}
extern "C" int ggml_hip_sampler_get_guidance(ggml_hip_sampler * s, int32_t * guide_row_out, float * scale_out) {
    if (!s) return 1;
    for (int r = 0; r < s->n_rows; ++r) {
        if (guide_row_out) guide_row_out[r] = s->guide_host[r];
        if (scale_out) scale_out[r] = s->scale_host[r];
    }
    return 0;
}

extern "C" void ggml_hip_sampler_sample(ggml_hip_sampler * s, const float * logits_dev, int64_t row_stride, int32_t * tokens_dev) {
    fq_launch_sample(s, s->n_rows, logits_dev, row_stride, tokens_dev, nullptr, nullptr, nullptr, 0, fq_ctx().stream);
}

// ---- draft and verify on caller-made logits (fq_spec.h)
extern "C" int ggml_hip_sampler_verify_rows(ggml_hip_sampler * s, const float * logits_dev, int64_t row_stride, int n_rows, const int32_t * drafts_dev,
                                            int32_t * out_dev, int32_t * n_out_dev) {
    if (!s || !logits_dev || !out_dev || !n_out_dev || n_rows < 1 || n_rows > FQ_SPEC_MAX_DRAFT + 1 || (n_rows > 1 && !drafts_dev)) {
        fprintf(stderr, "ggml-hip: sampler_verify_rows: %d rows (1..%d) or a missing argument\n", n_rows, FQ_SPEC_MAX_DRAFT + 1);
        return 1;
    }
    if (s->gram_host[0]) { fprintf(stderr, "ggml-hip: sampler_verify_rows: row 0 holds a grammar and a verify pass applies none: take it off first\n"); return 1; }
    spec_alloc(s);
    hipStream_t st = fq_ctx().stream;
    fq_spec_state fresh;
    fq_spec_reset(&fresh);
    HIP_CHECK(hipMemcpyAsync(s->spec_state, &fresh, sizeof fresh, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemsetAsync(s->spec_drafts, 0xff, FQ_SPEC_MAX_DRAFT * 4, st));
    if (n_rows > 1) HIP_CHECK(hipMemcpyAsync(s->spec_drafts, drafts_dev, (size_t)(n_rows - 1) * 4, hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipMemsetAsync(out_dev, 0xff, (size_t) n_rows * 4, st));
    HIP_CHECK(hipMemsetAsync(s->steps, 0, 4, st));
    const fq_spec_launch sp{ s->spec_state, nullptr, 0, nullptr, s->spec_drafts, nullptr, n_rows, FQ_SPEC_OFF, 1, 1, 0 };
    fq_launch_verify(s, sp, logits_dev, row_stride, s->tok, nullptr, s->steps, out_dev, st);
    HIP_CHECK(hipMemcpyAsync(n_out_dev, s->steps, 4, hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));                    // (fresh is a local)
    return 0;
}

extern "C" int ggml_hip_draft_lookup(const int32_t * history_dev, int n, int ngram_min, int ngram_max, int n_draft, int32_t * drafts_out_dev) {
    if (!drafts_out_dev || n < 0 || (n > 0 && !history_dev) || n_draft < 1 || n_draft > FQ_SPEC_MAX_DRAFT || ngram_min < 1 || ngram_max < ngram_min || ngram_max > FQ_SPEC_MAX_NGRAM) {
        fprintf(stderr, "ggml-hip: draft_lookup: n %d, n-grams %d..%d (1 <= min <= max <= %d), %d drafts (1..%d)\n", n, ngram_min, ngram_max, FQ_SPEC_MAX_NGRAM, n_draft, FQ_SPEC_MAX_DRAFT);
        return 1;
    }
    hipLaunchKernelGGL(k_draft_lookup, dim3(1), dim3(FQ_SK_THREADS), 0, fq_ctx().stream, history_dev, n, ngram_min, ngram_max, n_draft, drafts_out_dev);
    return 0;
}
