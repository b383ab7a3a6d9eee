/*
 * falcon-hip.h -- C ABI of libggml_hip.so, model level: a device-resident Falcon decoder stack.
 *
 * Mirrors the part of libfalcon.h that sits on the hot path (cmp-nct/ggllm.cpp):
 *   falcon_hip_model_*    <- falcon_model / falcon_model_load_internal   (libfalcon.cpp:1552-1959)
 *   falcon_hip_context_*  <- falcon_context_prepare / kv_cache_init      (libfalcon.cpp:3755, 1335-1385)
 *   falcon_hip_eval       <- falcon_eval -> falcon_eval_internal         (libfalcon.cpp:4566, 2011-2588)
 *   falcon_hip_get_logits <- falcon_get_logits                           (libfalcon.cpp:4678)
 * Unlike the reference (which rebuilds a ggml graph per call, runs attention/LN/GELU on the CPU and round-trips
 * every mat-mul over PCIe), all weights, the KV cache and every activation stay in HBM; only token ids go in and
 * logits come out. A context may own a contiguous range of layers (a pipeline STAGE): the first
 * stage embeds tokens, inner stages take/give the residual stream as device pointers, the last stage applies
 * ln_f + lm_head.
 */
#ifndef FALCON_HIP_H
#define FALCON_HIP_H

#include <stddef.h>
#include <stdint.h>
#include "ggml-hip-ops.h"         /* ggml_hip_sampling */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct falcon_hip_model   falcon_hip_model;
typedef struct falcon_hip_context falcon_hip_context;

typedef struct falcon_hip_hparams {      /* falcon_hparams, libfalcon.cpp:146-160 */
    int32_t n_vocab, n_embd, n_head, n_head_kv, n_layer, n_ff;
    int32_t two_norms;                   /* 1: ln_attn + ln_mlp per block (40B / 180B), 0: shared input_layernorm (7B) */
    int32_t layer_begin, layer_end;      /* this process holds blocks [layer_begin, layer_end)                         */
} falcon_hip_hparams;

falcon_hip_model * falcon_hip_model_create(const falcon_hip_hparams * hp);
void               falcon_hip_model_free(falcon_hip_model * m);
/* Upload one tensor by its model-file name (libfalcon.cpp:1764-1861), e.g.
 *   transformer.word_embeddings.weight, transformer.h.<i>.self_attention.query_key_value.weight,
 *   transformer.h.<i>.self_attention.dense.weight, transformer.h.<i>.mlp.dense_h_to_4h.weight,
 *   transformer.h.<i>.mlp.dense_4h_to_h.weight, transformer.h.<i>.input_layernorm.{weight,bias} (7B),
 *   transformer.h.<i>.ln_mlp.* / ln_attn.* (40B), transformer.ln_f.{weight,bias}, lm_head.weight
 * type: enum ggml_type value (0 = f32 for the norms; any matrix may be 1 = F16: row-major fp16, kept at 2 bytes per
 * weight and multiplied with the reference's f64 row sums, ggml_hip_mul_mat_f16). data: host bytes in ggml layout.
 * Returns 0, or -1 if the name is unknown / outside this stage's layer range (tensor ignored).                  */
int  falcon_hip_model_set_tensor(falcon_hip_model * m, const char * name, int type, const void * data, int64_t ne0, int64_t ne1);
size_t falcon_hip_model_weight_bytes(const falcon_hip_model * m);   /* weight bytes read per decoded token (F16: 2 per weight) */

/* The reference's model file format, GGCC v10 (what falcon_quantize writes and falcon_main loads; libfalcon.cpp:770-973).
 * falcon_hip_model_load_ggcc maps the file and uploads blocks [layer_begin, layer_end) (layer_end <= 0: all; a pipeline
 * stage passes its own range) plus the embedding (first stage) and ln_f + lm_head (last stage); the vocabulary and BPE
 * merges are skipped (the tokenizer is not on this path). Matrices may be quantized or F16 (falcon_convert.py's file as it
 * is, or a quantized file whose lm_head stayed F16: --leave-output-tensor); F32 matrices are refused. Blocks with an F16
 * matrix and models with an F16 lm_head run the op-by-op launch list. Returns NULL on error (message on stderr).
 * falcon_hip_ggcc_scan is the host-only part (no device needed): header + tensor directory (one text line per tensor:
 * "name ggml_type ne0 ne1 file_offset bytes"); returns the number of tensors or -1.                                  */
falcon_hip_model * falcon_hip_model_load_ggcc(const char * path, int layer_begin, int layer_end, falcon_hip_hparams * hp_out);
int  falcon_hip_ggcc_scan(const char * path, falcon_hip_hparams * hp_out, int * ftype_out, char * dir_out, size_t dir_cap);

/* Stage plan of a layer pipeline for a GGCC file (host-only): n_stages contiguous block ranges that minimise the weight
 * bytes the slowest stage streams per token (the last stage also streams ln_f + lm_head) -- what the reference's VRAM
 * planner decides per device (libfalcon.cpp:1660-1900) -- and the device bytes each stage needs (weights + embedding on
 * the first stage + n_streams x (KV cache of n_ctx positions + activations of n_batch tokens)). layer_begin / layer_end /
 * stage_bytes: n_stages entries. Returns 0, 1 if a stage needs more than vram_per_gpu (0 = no limit), -1 on error.       */
int  falcon_hip_plan_stages(const char * path, int n_stages, int n_ctx, int n_batch, int n_streams, size_t vram_per_gpu,
                            int * layer_begin, int * layer_end, size_t * stage_bytes);

/* falcon_model_quantize (libfalcon.h:176-179, libfalcon.cpp:3533-3743) for GGCC v10 files: writes path_out with every
 * 2-D "...weight" tensor converted to the tensor type of ftype (enum llama_ftype value: 0 f32, 1 f16, 2 Q4_0, 3 Q4_1,
 * 7 Q8_0, 8 Q5_0, 9 Q5_1, 10 Q2_K, 11-13 Q3_K, 14-15 Q4_K, 16-17 Q5_K, 18 Q6_K), lm_head.weight only when
 * quantize_output_tensor, already-quantized sources only when allow_requantize; the quantizers run on the device and the
 * file is byte-identical with the reference's. hist_out: NULL or 16 counters (the reference's printed histogram, summed
 * over tensors). Returns 0, or 1 after a message on stderr (the reference's convention); a failed run leaves no file.   */
int  falcon_hip_model_quantize(const char * path_in, const char * path_out, int ftype, int quantize_output_tensor,
                               int allow_requantize, int64_t * hist_out);

void falcon_hip_model_get_hparams(const falcon_hip_model * m, falcon_hip_hparams * hp_out);

/* n_ctx: KV capacity; n_batch: largest N of one eval; rope_n_ctx: the n_ctx handed to ggml_rope
 * (n_max_real_ctx or n_ctx, libfalcon.cpp:2229-2230)                                                           */
falcon_hip_context * falcon_hip_context_create(falcon_hip_model * m, int n_ctx, int n_batch, int rope_n_ctx);
void                 falcon_hip_context_free(falcon_hip_context * c);
/* A context of n_seq (1..256) independent sequences that advance in LOCK STEP: every falcon_hip_eval_stage / falcon_hip_stage_step
 * evaluates n_seq rows = one token of each sequence, all at position n_past, row t attending to its own KV cache. One pass
 * over the weights serves n_seq tokens. n_seq <= 4 (k-quant models at model widths: <= 2): the column mat-vec kernels, the same
 * bits per sequence as a context of its own; more: the small-batch mat-muls (5..16 columns per pass, larger contexts in
 * passes of 16 or through the tile GEMM) -- a sequence's logits then equal a context of its own within the association
 * spread of the f32 sums (a row of those mat-muls does not depend on the other rows).
 * token_dev / next_token_dev of falcon_hip_stage_step then hold n_seq ids, the hidden rows are [n_seq][n_embd].          */
falcon_hip_context * falcon_hip_context_create_seqs(falcon_hip_model * m, int n_ctx, int n_seq, int rope_n_ctx);
int                  falcon_hip_context_n_seq(const falcon_hip_context * c);

/* Evaluate n_tokens at position n_past (falcon_eval). Whole model in this process: tokens are host ids.
 * logits_all = 0 keeps the last row only. Returns 0; 1 for an empty / oversized batch or a position past n_ctx (nothing is
 * evaluated), 2 for a token id outside the vocabulary, 3 if an in-launch hand-off timed out (results invalid).          */
int falcon_hip_eval(falcon_hip_context * c, const int32_t * tokens, int n_tokens, int n_past, int logits_all);
/* Pipeline-stage form: hidden_in_dev / hidden_out_dev are device [n_tokens][n_embd] f32 (NULL where the stage
 * embeds tokens / produces logits).                                                                             */
int falcon_hip_eval_stage(falcon_hip_context * c, const int32_t * tokens, const float * hidden_in_dev, int n_tokens,
                          int n_past, int logits_all, float * hidden_out_dev);
/* One decode step (N = 1) of a pipeline stage with device-resident inputs/outputs, asynchronous on the library stream:
 * token_dev (stage 0) or hidden_in_dev [n_embd] (other stages) -> hidden_out_dev [n_embd] (not the last stage) or the
 * greedy-sampled next_token_dev (last stage). The caller exchanges them with RCCL send/recv (bench_pipeline.py).      */
int falcon_hip_stage_step(falcon_hip_context * c, const int32_t * token_dev, const float * hidden_in_dev, int n_past,
                          float * hidden_out_dev, int32_t * next_token_dev);
/* Greedy decode loop entirely stream-ordered: evaluates `first_token` at n_past, then n_steps-1 more argmax-sampled
 * tokens (falcon_main --temp 0, falcon_main.cpp:958-960); out_tokens receives n_steps ids. No host sync per step. */
int falcon_hip_decode_greedy(falcon_hip_context * c, int32_t first_token, int n_past, int n_steps, int32_t * out_tokens);

/* RAGGED lock-step steps: row t is one token of sequence t at its own position n_past[t] -- rotated with the RoPE row of n_past[t],
 * its key and value appended at n_past[t] of its own cache, attending to keys [0, n_past[t]] of that cache. A row's logits are those of
 * the same row in a uniform step (all sequences at one position) of a context of the same n_seq whose sequences hold that row's cache
 * prefix and token. A context made by falcon_hip_context_create is a context of one sequence (seq 0).
 * falcon_hip_eval_seqs: one token per sequence (host arrays of n_seq); whole model in this process (1 otherwise). Logits of all n_seq
 * rows: falcon_hip_get_logits. Returns as falcon_hip_eval: 1 (nothing evaluated) if any n_past[t] < 0 or n_past[t] + 1 > n_ctx, 2 for
 * a token outside the vocabulary, 3 sticky hand-off error. */
int falcon_hip_eval_seqs(falcon_hip_context * c, const int32_t * tokens, const int32_t * n_past);
/* falcon_hip_decode_greedy per sequence: evaluates first_tokens[t] at n_past[t], then n_steps-1 argmax tokens; out_tokens [n_steps][n_seq];
 * stream-ordered, no host sync per step; honours falcon_hip_context_use_graph (one hipGraph replay per step, positions read from and
 * advanced in a device array). 1 if any n_past[t] + n_steps > n_ctx (or n_steps < 1), 2 and 3 as falcon_hip_eval_seqs. */
int falcon_hip_decode_greedy_seqs(falcon_hip_context * c, const int32_t * first_tokens, const int32_t * n_past, int n_steps, int32_t * out_tokens);
/* K and V rows [0, n_tokens) of every local layer: sequence src_seq of src -> sequence dst_seq of dst (stream-ordered). 1 (nothing copied)
 * unless both contexts hold the same falcon_hip_model and the same RoPE table (rope_n_ctx bucket), 0 <= seq < n_seq on each side and
 * n_tokens <= both n_ctx. How a prompt enters a running batch: prefill it in an ordinary context, copy its cache into a free slot. */
int falcon_hip_context_copy_seq(falcon_hip_context * dst, int dst_seq, const falcon_hip_context * src, int src_seq, int n_tokens);

/* SAMPLED decode: falcon_main's default sampler chain on the device (ggml_hip_sampling, include/ggml-hip-ops.h). Every sequence
 * of a context (one for falcon_hip_context_create) owns a sampler row -- parameters, window of recent tokens, mt19937 -- kept in
 * device memory across calls (two calls of 4 steps draw what one call of 8 does). Rows start greedy with an empty window.
 * falcon_hip_context_set_sampling: row `seq`'s parameters, seeded generator and window (the last repeat_last_n of n_ctx zeros
 * followed by history, as falcon_main's last_n_tokens); 0, or 1 (refused) as ggml_hip_sampler_set_row or for a bad seq.        */
int falcon_hip_context_set_sampling(falcon_hip_context * c, int seq, const ggml_hip_sampling * params, const int32_t * history, int n_history);
/* the same with tail-free, typical and mirostat 1 / 2 honoured (ggml_hip_sampling_ext, ggml_hip_sampler_set_row_ext: its contract,
 * limit and refusals); the sampled loops below then run those branches in the same captured step. get_mirostat_mu: mu_out [n_seq], each
 * sequence's mirostat state (2 * tau when set, moved by every draw; waits for the stream); 0, or 1 without an lm_head.            */
int falcon_hip_context_set_sampling_ext(falcon_hip_context * c, int seq, const ggml_hip_sampling_ext * params, const int32_t * history, int n_history);
int falcon_hip_context_get_mirostat_mu(falcon_hip_context * c, float * mu_out);
/* sequence src_seq's sampler row of src (parameters, window, generator state) -> sequence dst_seq of dst (ggml_hip_sampler_copy_row):
 * with falcon_hip_context_copy_seq, how a prompt drawn from in its own context continues its stream in a lock-step slot. 0, or 1.  */
int falcon_hip_context_copy_sampling(falcon_hip_context * dst, int dst_seq, falcon_hip_context * src, int src_seq);
/* one draw per sequence from the last eval's logits: row N-1 after falcon_hip_eval of N tokens (or falcon_hip_eval_token), row t for
 * sequence t after falcon_hip_eval_seqs; out [n_seq]. The drawn token enters the row's window. 0, or 1 without an lm_head.        */
int falcon_hip_sample(falcon_hip_context * c, int32_t * out);
/* falcon_hip_decode_greedy / falcon_hip_decode_greedy_seqs with the sampler chain in place of the argmax: the same contracts and
 * return codes, falcon_hip_context_use_graph honoured (one replay per step). first_token(s) do not enter the window (they entered
 * it when drawn, or with the history); every drawn token does.                                                              */
int falcon_hip_decode_sample(falcon_hip_context * c, int32_t first_token, int n_past, int n_steps, int32_t * out_tokens);
int falcon_hip_decode_sample_seqs(falcon_hip_context * c, const int32_t * first_tokens, const int32_t * n_past, int n_steps, int32_t * out_tokens);
/* Log-probabilities of what the sampled loops generate (ggml_hip_logprob_rows, ggml-hip-ops.h). n_top: -1 off (the default), 0 the
 * chosen token's probability only, 1..32 also the n_top most likely ids with theirs. While on, falcon_hip_sample,
 * falcon_hip_decode_sample and falcon_hip_decode_sample_seqs launch the kernel behind the sampler's launch, on the same stream
 * (one more node of the captured step), and keep the records on the device, laid out like the token output: prob [n_steps][B],
 * top ids and probabilities [n_steps][B][n_top] (B = the context's sequences; falcon_hip_sample: one step). The probabilities are
 * those of the raw logits row the token was drawn from -- what falcon_hip_eval_score gives for that token -- not of the sampler's
 * edited distribution. Off: nothing is allocated or launched, the loops are what they were. The greedy loops
 * (falcon_hip_decode_greedy[_seqs]), pipeline stages and the link-time wrap record nothing: greedy generation with
 * log-probabilities is the sampled loop at temp <= 0. set: 1 (message) for n_top outside [-1, 32], above n_vocab, or a context
 * without lm_head. get: copies the records of the last such call to the host (top_* may be NULL); 1 if off or no such call has
 * run since the setting changed or since a greedy loop.                                                                   */
int falcon_hip_context_set_logprobs(falcon_hip_context * c, int n_top);
int falcon_hip_get_logprobs(falcon_hip_context * c, float * prob_out, int32_t * top_id_out, float * top_prob_out);
/* STOPS: the sampled loops end a sequence on the device (ggml_hip_stops, ggml_hip_sampler_set_stops in ggml-hip-ops.h: up to 16 stop
 * sequences of 1..8 token ids and a budget max_tokens of drawn tokens per sequence). Off by default; while no sequence of a context has
 * stops, its loops launch, capture and return what they did before. Drawn tokens are those falcon_hip_sample or a sampled loop drew
 * for the sequence since its stops were set: first_token(s) and the history of set_sampling are not (the rule of the penalty window).
 * The state (drawn count, the last 8 drawn tokens, the reason) persists across calls, so a sequence whose tokens two consecutive loop
 * calls drew still matches. A sequence ends AT the draw that completes a stop sequence (reason: its index, the lowest if several) or
 * reaches the budget (GGML_HIP_STOP_BUDGET); falcon_main notices a stopword one iteration later and also looks at prompt tokens.
 * From then on the sequence is FROZEN until its stops are set again: nothing is drawn for it, and its generator, window, token,
 * position, step counter and log-probability records stay as they are -- clear or set its stops and call a loop with its last token at
 * its position to continue exactly where it ended. With stops on any sequence of the context the sampled loops fill out_tokens with -1
 * first: out_tokens[s][t] == -1 for every step past sequence t's end (the token that ended it is written). A frozen sequence still
 * rides the lock-step pass: its token is evaluated again at its position, which rewrites the same K / V row. Log-probability records
 * past a sequence's end are unspecified; those up to and including the token that ended it are kept. Return codes and the shapes
 * falcon_hip_get_logprobs copies are unchanged.
 * When EVERY sequence of the context has stops the loop also ends early: after every `every_steps` steps (set_stop_poll; default 16:
 * measured no dearer than 4 or 64, see csrc/falcon_ctx.h) it copies the sequences' states to the host behind the steps and, two chunks later, stops
 * enqueuing once all have ended; if the last sequence ends at step k (0-based) at most (k / every_steps + 2) * every_steps steps are
 * launched. falcon_hip_context_loop_steps: the steps the last decode loop launched (a diagnostic).
 * set_stops: sequence seq's stops (NULL: off); the state starts afresh, generator and window are untouched. Turning stops on or off
 * for a context re-captures its sampled step; changing a sequence's stops does not. 0, or 1 (refused, nothing changed) as
 * ggml_hip_sampler_set_stops. get_stops: [n_seq] drawn counts and reasons (GGML_HIP_STOP_RUNNING while running or off); waits for
 * the stream. falcon_hip_context_copy_sampling carries a sequence's stops and their state with the row: a prompt whose first token
 * was drawn in its own context continues in a lock-step slot with its budget and tail intact. falcon_hip_sample honours the stops
 * (out[t] = -1 for a sequence that had ended before the call).
 * The greedy loops (falcon_hip_decode_greedy[_seqs]), pipeline stages and the link-time wrap ignore them: greedy generation with
 * stops is the sampled loop at temp <= 0.                                                                                    */
int  falcon_hip_context_set_stops(falcon_hip_context * c, int seq, const ggml_hip_stops * stops);
int  falcon_hip_context_get_stops(falcon_hip_context * c, int32_t * n_drawn_out, int32_t * reason_out);
void falcon_hip_context_set_stop_poll(falcon_hip_context * c, int every_steps);   /* >= 1 (smaller: 1) */
int  falcon_hip_context_loop_steps(const falcon_hip_context * c);

/* falcon_eval with n_tokens = 1 (libfalcon.cpp:4566) without a host round trip: the fused decode launches are replayed from a
 * hipGraph and the logits row is copied into page-locked host memory behind them; falcon_hip_get_logits waits for that copy
 * (libfalcon.h:256, 263). Returns as falcon_hip_eval; an in-launch hand-off that timed out in such an asynchronous step is
 * noticed at the next falcon_hip_get_logits and is STICKY: falcon_hip_context_last_error reports 3 and every later eval of the
 * context returns 3 (its KV cache holds invalid rows). */
int falcon_hip_eval_token(falcon_hip_context * c, int32_t token, int n_past);
int falcon_hip_context_last_error(const falcon_hip_context * c);      /* 0 or 3; host state only (no device wait) */
/* the n_ctx ggml_rope is given may change per call (falcon_evaluation_config::n_max_real_ctx, libfalcon.cpp:2229-2230);
 * the table is rebuilt when the dynamic-NTK bucket n_ctx / 2048 changes (<= 0: the context's n_ctx)                       */
void falcon_hip_context_set_rope_n_ctx(falcon_hip_context * c, int rope_n_ctx);
/* falcon_hip_eval, then one line per launch site on stderr (calls, total / average microseconds, share): what the reference's --debug-timings node table
 * (libfalcon.cpp:2506-2520) becomes on the resident path, where a block is a handful of launches instead of a ggml graph; falcon_wrap.cpp calls it where the
 * reference would print its table (falcon_evaluation_config::debug_timings, same first / last / every-token rule) */
int   falcon_hip_eval_debug_timings(falcon_hip_context * c, const int32_t * tokens, int n_tokens, int n_past, int logits_all);
const float * falcon_hip_get_logits(falcon_hip_context * c);        /* host, n_vocab (or n_tokens*n_vocab) floats; NULL after falcon_hip_eval_score */
/* falcon_hip_eval of n_tokens at n_past with the logits of every row kept on the device, then probs_out[r] (host) = the
 * reference's soft-max probability of targets[r] in row r, for every r with targets[r] >= 0 (other entries untouched).
 * The arithmetic is falcon_perplexity.cpp:12-27 (ggml_hip_score_rows, ggml-hip-ops.h): the bits the host loop over
 * falcon_hip_eval(..., 1) + falcon_hip_get_logits gives, with n_tokens floats instead of n_tokens * n_vocab crossing the bus.
 * Returns as falcon_hip_eval; 2 as well if a target is >= n_vocab (nothing evaluated), 1 for a context without lm_head, a
 * pipeline stage or a lock-step context. Afterwards falcon_hip_get_logits returns NULL (nothing was copied);
 * falcon_hip_sample draws from the last row as after falcon_hip_eval.                                                  */
int falcon_hip_eval_score(falcon_hip_context * c, const int32_t * tokens, int n_tokens, int n_past,
                          const int32_t * targets, float * probs_out);
/* The reference's perplexity loop (falcon_perplexity.cpp:28-124) over a token stream: chunks of n_ctx tokens evaluated
 * from an empty context in batches of n_batch, NLL of the second half of every chunk (soft_max as in :12-27, on the device:
 * falcon_hip_eval_score per batch; -log(prob) and the running sum on the host, in position order).
 * Returns the number of scored tokens and their summed NLL (perplexity = exp(nll / count)).                            */
int   falcon_hip_perplexity(falcon_hip_context * c, const int32_t * tokens, int64_t n_tokens, int n_ctx, int n_batch, double * nll_out);
/* ---- embeddings (falcon_get_embeddings, libfalcon.cpp:2409-2435, 2551-2557; pooled vectors: csrc/kernels_embed.hip, csrc/fq_embed.h).
 * falcon_hip_context_set_embedding: mode is a bit set -- FALCON_HIP_EMBED_LAST: every falcon_hip_eval / _eval_score / _embed keeps the ln_f row of its
 * last token (what the reference fills ctx->embedding with under params.embedding); FALCON_HIP_EMBED_POOL: the ln_f rows of every token are also summed,
 * per column in f64 and in position order, until falcon_hip_embedding_pool_reset. 0 (the default) switches both off: every call then launches exactly
 * what it launched before the mode was set, from the same captured graphs. Returns 0, or 1 after a message with nothing changed for a lock-step
 * context, a pipeline stage, a row-split model or an unknown bit. While a mode is set the decode loops (falcon_hip_decode_*), falcon_hip_context_swap and
 * falcon_hip_perplexity refuse with a message (the reference's loops never see the embedding either: falcon_main refuses --embedding), and the state
 * blob and session file carry the row (below).
 * falcon_hip_get_embeddings: n_embd floats on the host, valid until the next eval; NULL while FALCON_HIP_EMBED_LAST is off or before the first eval.
 * In reference orders 1 and 2 the row is the reference's bit for bit.
 * falcon_hip_embed: falcon_hip_eval that ends after ln_f -- K / V are written as by falcon_hip_eval (a text longer than n_batch is a sequence of calls),
 * lm_head is not run and falcon_hip_get_logits returns NULL afterwards. Returns as falcon_hip_eval, 1 while no mode is set.
 * falcon_hip_get_embedding_pooled: out (host, n_embd floats) = the mean of the pooled rows, (float)(sum / count), or with normalize that mean divided in
 * f64 by its f64 Euclidean length. 1 when nothing was pooled, 2 when the mean is the zero vector, 3 without FALCON_HIP_EMBED_POOL: out untouched.
 * falcon_hip_embedding_pool_count: rows pooled since the last reset.                                                                                  */
#define FALCON_HIP_EMBED_LAST 1
#define FALCON_HIP_EMBED_POOL 2
int   falcon_hip_context_set_embedding(falcon_hip_context * c, int mode);
const float * falcon_hip_get_embeddings(falcon_hip_context * c);
int   falcon_hip_embed(falcon_hip_context * c, const int32_t * tokens, int n_tokens, int n_past);
int   falcon_hip_embedding_pool_reset(falcon_hip_context * c);
int   falcon_hip_get_embedding_pooled(falcon_hip_context * c, int normalize, float * out);
int64_t falcon_hip_embedding_pool_count(const falcon_hip_context * c);
/* test hook: residual stream entering each local layer (+ leaving the last), device->host, after an eval with
 * falcon_hip_context_keep_hidden(c, 1): (n_local_layers + 1) * n_tokens * n_embd floats                          */
void  falcon_hip_context_keep_hidden(falcon_hip_context * c, int keep);
void  falcon_hip_get_hidden(falcon_hip_context * c, float * dst_host);
void  falcon_hip_context_use_graph(falcon_hip_context * c, int enable);   /* the decode loops replay one captured step (a hipGraph) per token; re-captured by itself whenever a mode, a global switch or a buffer it was captured with changes */
int   falcon_hip_context_graph_captures(const falcon_hip_context * c);    /* test and diagnostic hook: hipGraph captures of this context so far */
/* N == 1 evals: 2 (default) = fused decode kernels, two launches per block (LayerNorm mat-vec in the ring form, csrc/kernels_ring.hip, where the format has it |
 * attention + output mat-vec, when the grid fits the chip), 3 = one launch per block (the next block's LayerNorm mat-vec as a second phase of the same
 * launch; measured slower, kept for A/B), 1 = three launches, 0 = one launch per graph op (tests), 5 = mode 2 with the ring form forced. All produce the
 * same bits. (4 was the persistent decode engine of rounds 2-3 -- one launch per token, measured 36 % slower, removed in round 6: it now selects mode 2.)
 * With ggml_hip_reference_order(2) (ggml-hip-ops.h) modes 1, 2 and 5 run the same launches in the reference's own association (csrc/fq_ref_chain.h). */
void  falcon_hip_context_set_fused(falcon_hip_context * c, int mode);
/* 1 if an in-launch wait of the 2-launch form ever timed out (results invalid; never expected). Synchronises the device. */
int   falcon_hip_context_sync_error(falcon_hip_context * c);

/* ---- layer pipeline over several GPUs, one process per GPU (csrc/falcon_pipeline.hip). Rank r holds the blocks
   [layer_begin, layer_end) of its falcon_hip_model (falcon_hip_plan_stages picks the ranges); n_groups groups of `batch`
   lock-step sequences are in flight (n_groups >= world; >= 2 x world: transfers overlap stage steps); the residual rows and
   the sampled tokens travel by RCCL ncclSend / ncclRecv (xGMI). What the reference does instead: every mat-mul split over the
   devices with peer copies and a gather on the main device (ggml-cuda.cu:2586-2608, 2713-2732).
     rank 0:  falcon_hip_pipeline_unique_id(id)  -> hand the 128 bytes to the other ranks (launcher's store, file, MPI ...)
     all:     p = falcon_hip_pipeline_create(model, rank, world, id, n_groups, batch, n_ctx)
     rank 0:  falcon_hip_pipeline_set_tokens(p, first_tokens)            n_groups * batch ids (sequence i = group * batch + b)
     all:     falcon_hip_pipeline_run(p, rounds, n_past0)                 asynchronous; every sequence advances `rounds` tokens
     last:    falcon_hip_pipeline_get_history(p, out, first_round, n)     the sampled tokens [round][sequence]; waits
   world == 1 needs neither RCCL nor an id (NULL). */
#define FALCON_HIP_PIPELINE_ID_BYTES 128
typedef struct falcon_hip_pipeline falcon_hip_pipeline;
int   falcon_hip_pipeline_unique_id(void * id_out);                       /* 0, or -1 when RCCL is not available */
falcon_hip_pipeline * falcon_hip_pipeline_create(falcon_hip_model * m, int rank, int world, const void * unique_id,
                                                 int n_groups, int batch, int n_ctx);
void  falcon_hip_pipeline_free(falcon_hip_pipeline * p);
int   falcon_hip_pipeline_rccl_ranks(falcon_hip_pipeline * p);           /* ncclCommCount of its communicator (1: one rank, 0: local transport) */
/* how this rank's hand-offs travel: 0 one stage (none), 1 RCCL ncclSend / ncclRecv, 2 device copies inside one process (local), 3 the local job over
 * a one-rank RCCL communicator, 4 host shared memory between the processes of one node -- selected for falcon_hip_pipeline_create by the environment,
 * FALCON_PIPE_TRANSPORT=shm: the multi-process job on a node whose ranks share a GPU (RCCL refuses two ranks on one device); same ranks, same unique-id
 * hand-out, same slot schedule and stage steps, the exchange blocking on the host */
int   falcon_hip_pipeline_transport(falcon_hip_pipeline * p);
/* one small message around the ring of ranks over a fresh RCCL communicator (rank r -> r + 1), checked and torn down: 0 = RCCL's send / recv works between
 * these ranks. bench_pipeline.py runs it in a child process per rank under a time-out before the job and falls back to FALCON_PIPE_TRANSPORT=shm otherwise. */
int   falcon_hip_rccl_selftest(int rank, int world, const void * unique_id, int device);
int   falcon_hip_pipeline_set_tokens(falcon_hip_pipeline * p, const int32_t * tokens);
int   falcon_hip_pipeline_run(falcon_hip_pipeline * p, int rounds, int n_past0);
int   falcon_hip_pipeline_get_history(falcon_hip_pipeline * p, int32_t * out, int first_round, int n_rounds);
/* the same job with every rank inside ONE process on one device (hand-off by device copies instead of RCCL): the identical
   schedule and stage code, for tests and for sizing a pipeline before the GPUs are there */
falcon_hip_pipeline * falcon_hip_pipeline_create_local(falcon_hip_model * m, int rank, int world, int n_groups, int batch, int n_ctx);
int   falcon_hip_pipeline_run_local(falcon_hip_pipeline ** ranks, int world, int rounds, int n_past0);
/* switches a local job's hand-offs from device copies to RCCL itself: one communicator of ONE rank (this process and GPU), every
   message a grouped ncclSend / ncclRecv addressed to rank 0 on the pipeline's second stream, ordered by the events of the overlapped
   schedule -- the library's RCCL binding and call sequence exercised on a box with a single GPU. 0, or -1 (RCCL missing / refused);
   afterwards falcon_hip_pipeline_rccl_ranks reports the communicator's count (1) for every rank of the job */
int   falcon_hip_pipeline_local_attach_rccl(falcon_hip_pipeline ** ranks, int world);
/* host only: the slot schedule (see falcon_pipeline.hip); out: 9 ints; returns the number of slots of the run */
int   falcon_hip_pipeline_schedule(int rank, int world, int n_groups, int rounds, int slot, int * out);

/* ---- tokenizer (host only): falcon_tokenize / falcon_token_to_str (libfalcon.h:236-247, libfalcon.cpp:2594-3035, 4623-4641)
   on the vocabulary and BPE merges stored in a GGCC v10 file. Same ids as the reference for any text. */
typedef struct falcon_hip_vocab falcon_hip_vocab;
falcon_hip_vocab * falcon_hip_vocab_load_ggcc(const char * path);          /* never NULL; check falcon_hip_vocab_error */
const char * falcon_hip_vocab_error(const falcon_hip_vocab * v);           /* NULL = loaded */
void  falcon_hip_vocab_free(falcon_hip_vocab * v);
int   falcon_hip_vocab_size(const falcon_hip_vocab * v);
int   falcon_hip_vocab_merges(const falcon_hip_vocab * v);
/* ids of `text` (bos = 11 first when add_bos and the text is not empty); returns their number, or minus that number when
   n_max is too small (nothing written), as falcon_tokenize does */
int   falcon_hip_tokenize(const falcon_hip_vocab * v, const char * text, int32_t * tokens, int n_max, int add_bos);
/* the token's bytes (not NUL-terminated: byte tokens may be 0); returns their number or -1 */
int   falcon_hip_token_to_bytes(const falcon_hip_vocab * v, int32_t id, const char ** bytes);
int32_t falcon_hip_token_bos(void);
int32_t falcon_hip_token_eos(void);

/* ---- STOP STRINGS: the sampled loops end a sequence on the bytes it generated (ggml_hip_stop_text, ggml_hip_sampler_set_stop_text in
 * ggml-hip-ops.h hold the rule: up to 16 strings of 1..32 bytes per sequence, matched against the concatenated bytes of the tokens drawn
 * since the sequence's stops were set -- first_token(s) and set_sampling's history do not count -- the earliest completing byte winning,
 * then the lowest string index). `--stop "User:"` as ids misses " User" + ":", ".\n\n" + "User:" and a long token with the text in its
 * middle; the bytes do not. Off by default, and off means the loops launch, capture and return what they did before.
 * falcon_hip_model_set_vocab: the bytes of every token of v (what falcon_hip_token_to_bytes returns) as device arrays, built once
 * and shared by all contexts of the model, also those made before. 0, or 1 after a message, nothing changed, for a vocabulary whose
 * size differs from the model's n_vocab, a model without lm_head, or bytes beyond 16 MB. Setting it again replaces the arrays (the
 * sampled steps re-capture); v need not outlive the call.
 * falcon_hip_context_set_stop_text: sequence seq's strings (NULL: off). Turns the sequence's stops on -- zero id sequences and no
 * budget unless falcon_hip_context_set_stops gave some -- and starts the whole shared state afresh (drawn count, reason, id tail,
 * byte ring, cut_bytes); set_stops on a sequence with strings does the same. 0, or 1 (refused, nothing changed): n outside 0..16, a
 * length outside 1..32, no vocabulary set on the model, a context without lm_head, a bad sequence.
 * The reason arrives through falcon_hip_context_get_stops as GGML_HIP_STOP_TEXT0 + k (16..31: values that cannot appear unless
 * strings are set). falcon_hip_context_get_stop_text: cut_bytes_out [n_seq] -- the bytes from the first byte of the match to the end of
 * the sequence's drawn text, 0 while it has not ended by text: the detokenised drawn tokens minus cut_bytes bytes is the text before
 * the stop string. Order on one draw: id sequences, budget, strings; a text match replaces a budget end, never an id match.
 * Everything said of an ended sequence above holds (frozen, -1 past its end, the loop's early end: it reads the same reason word).
 * Turning strings on or off for a context re-captures its sampled step once; changing strings does not (they are device data).
 * falcon_hip_context_copy_sampling carries strings, ring and cut_bytes: a stop text may begin in the prompt's own context and end in a
 * lock-step slot. The greedy loops, pipeline stages and the link-time wrap ignore stop strings as they ignore id stops.          */
int   falcon_hip_model_set_vocab(falcon_hip_model * m, const falcon_hip_vocab * v);
int   falcon_hip_context_set_stop_text(falcon_hip_context * c, int seq, const ggml_hip_stop_text * text);
int   falcon_hip_context_get_stop_text(falcon_hip_context * c, int32_t * cut_bytes_out);

/* ---- GRAMMARS: constrained decoding inside the sampled loops (ggml_hip_dfa, ggml_hip_grammar_create, ggml_hip_sampler_set_grammar in
 * ggml-hip-ops.h hold the rule: a byte automaton; at every draw the sequence behaves as if it had a -inf logit bias on every token the
 * automaton forbids in its state, and the state moves with the drawn token's bytes; eos_id is allowed exactly in accepting states).
 * "One of these strings", "a number", "JSON of this shape" stay inside the captured step: no logits row crosses to the host.
 * falcon_hip_grammar_create: the grammar over the vocabulary of falcon_hip_model_set_vocab (the grammar keeps its own copy, so index
 * and advance never see different vocabularies). NULL after a message, nothing left behind: no vocabulary on the model, or as
 * ggml_hip_grammar_create (ggml_hip_grammar_last_error, *bad_state). One grammar serves any number of sequences and contexts of
 * models with that vocabulary. falcon_hip_grammar_free: 0, or 1 (refused) while a sequence holds it.
 * falcon_hip_context_set_grammar: sequence seq's grammar (NULL: none) and state (-1: the start state). 0, or 1 (refused, nothing
 * changed): a state out of range, a bad sequence, a context without lm_head, or draft-and-verify decode on -- a verify pass applies no
 * grammar, and falcon_hip_context_set_spec on a context with a grammar is refused likewise. Turning the first grammar of a context on or
 * the last off re-captures its sampled step once; another grammar or state does not (device data).
 * falcon_hip_context_get_grammar_state: states_out [n_seq], -1 for sequences without a grammar; waits for the stream.
 * A sequence that ends at a draw (stops, strings, budget, end of the cache) has the state that includes that draw; frozen, its state
 * stays. falcon_hip_context_copy_sampling carries grammar and state into a lock-step slot; falcon_hip_context_swap leaves both alone
 * (the evaluated-again tokens were drawn under the grammar already). With EOS among the stops a completed match ends the sequence one
 * step later, EOS being the only allowed token; there is no stop reason of its own.
 * Not covered: the fused-argmax greedy loops (use temp <= 0 in the sampled loops), pipeline stages, the link-time wrap.           */
ggml_hip_grammar * falcon_hip_grammar_create(falcon_hip_model * m, const ggml_hip_dfa * dfa, int eos_id, int * bad_state);
int   falcon_hip_grammar_free(ggml_hip_grammar * g);
int   falcon_hip_context_set_grammar(falcon_hip_context * c, int seq, ggml_hip_grammar * g, int state);
int   falcon_hip_context_get_grammar_state(falcon_hip_context * c, int32_t * states_out);

/* ---- CONTEXT SWAP: generate past n_ctx the way falcon_main does (examples/falcon/falcon_main.cpp:694-751; csrc/fq_ctx_swap.h restates
 * the rule). When its cache is full falcon_main keeps the system prompt and --keep tokens, evaluates a tail of what it generated again
 * behind them and goes on, so -n may be any size. Three pieces: a planner on the host, a stop at the end of the cache inside the sampled
 * loops, and the swap that regenerates and lets the sequence run again. The caller's loop:
 *     loop (falcon_hip_decode_sample[_seqs]) -> sequence ends with GGML_HIP_STOP_CONTEXT -> falcon_hip_swap_plan -> falcon_hip_context_swap
 *     -> loop again with first token = the waiting token (the sequence's last output) and n_past = n_past_new + n_regen.
 * falcon_hip_swap_plan (host only, no device needed): with the cache full and the last n_pending tokens of the history not evaluated yet
 * (1 while generating: the token just drawn),
 *     n_keep  := (n_keep < 0 || n_keep > prompt_size) ? prompt_size : n_keep          (prompt_size counts the system tokens)
 *     *n_past_new := n_system + ((n_keep > 0 && prompt_size > n_system) ? min(n_keep, prompt_size - n_system) : 0)
 *     *n_regen := *n_past_new < n_ctx/2 ? n_ctx/2 - *n_past_new : (*n_past_new < n_ctx - 10 ? 4 : 0), at most n_history - n_pending
 * and the regenerated tokens are history[n_history - n_pending - *n_regen .. n_history - n_pending). 0, or 1 with nothing written for
 * n_ctx < 1, negative sizes, n_system > prompt_size or n_pending outside 0..n_history.
 * The history is falcon_main's all_generation and NOT prompt + generation: the LAST token of every prompt batch of n_batch tokens, then
 * every drawn token, the waiting one included. falcon_hip_swap_history writes the part a prompt leaves -- (n_prompt + n_batch - 1) /
 * n_batch tokens, returned; history_out may be NULL to ask for the count -- and the caller appends what it draws. With a long prompt
 * and a short generation the clamp above pulls such batch-last prompt tokens into the regenerated tail; that is reproduced.
 * falcon_hip_context_set_context_stop(c, on): off by default, and off means the loops launch, capture, refuse and return what they did
 * before. On: every sequence of the context has stops (zero id sequences, no budget, unless set_stops / set_stop_text gave some; a
 * sequence that had none starts from a fresh state), and falcon_hip_decode_sample[_seqs] accept n_past + n_steps > n_ctx (every sequence
 * still needs n_past < n_ctx). The draw made at position n_ctx - 1 fills the cache: the sequence does not move -- its tokens_dev entry
 * and position stay, so riding on frozen through the lock-step pass it evaluates the same token at the same position again -- and, if
 * no other rule ended it at that draw (order: id sequences, budget, strings, then this), it ends with GGML_HIP_STOP_CONTEXT. The drawn
 * token has entered the window, the id tail and the byte ring, counts in n_drawn and is the sequence's last output: it is falcon_main's
 * pending token. No position >= n_ctx is ever evaluated or written. Turning it on or off re-captures the sampled step once. The greedy
 * loops ignore it as they ignore stops (greedy past n_ctx is the sampled loop at temp <= 0); falcon_hip_sample knows no position and
 * ignores it too. 0, or 1 for a context without lm_head.
 * falcon_hip_context_resume(c, seq): a sequence that ended with GGML_HIP_STOP_CONTEXT runs again; nothing else changes -- not n_drawn,
 * the id tail, the byte ring, cut_bytes, the generator, the window or mirostat's mu: a stop sequence or string may straddle the swap and
 * a budget spans it. 0, or 1 (message, nothing changed) for any other reason.
 * falcon_hip_context_swap: evaluates regen[0 .. n_regen) at positions n_past_new .. of sequence seq's cache, in chunks of at most n_batch
 * (and of the context's n_batch) from the front through the prefill path, then resumes the sequence. Untouched: rows [0, n_past_new) bit
 * for bit, every sampler state, every other sequence's cache and state; no standing buffer moves, so
 * falcon_hip_context_graph_captures does not grow across swaps. A lock-step context evaluates in a plain context of the same n_ctx that
 * the library makes at the context's first swap and keeps until it is freed -- ONE MORE KV CACHE of n_ctx rows plus n_batch rows of
 * activations -- with the kept rows copied in and the regenerated rows copied back.
 * What the REFERENCE keeps differs, and reference orders 1 and 2 (ggml_hip_reference_order) follow it: it stores V transposed and packed
 * to the current length and re-packs it at every eval from a view of stride n_past (libfalcon.cpp:2255-2281); behind a swap that view
 * has the kept length's stride over a buffer packed for n_ctx, so its "kept" V element (t, hd) is element hd * n_past_new + t of the
 * packed buffer. In those orders the swap first re-packs V rows [0, n_past_new) of the sequence the same way (K stays), and the
 * continuation is the reference's token for token also with kept rows; in the default order the rows stay bit for bit as said above.
 * Returns 0; 1 (message, nothing changed) for a
 * pipeline stage, a bad sequence, n_past_new + n_regen + 1 > n_ctx, n_batch < 1 or a sequence that did not end with
 * GGML_HIP_STOP_CONTEXT; 2 for a token id outside the vocabulary; 3 as falcon_hip_eval.                                          */
typedef struct falcon_hip_swap_cfg {
    int32_t n_ctx;          /* the context's length */
    int32_t n_system;       /* tokens of the system prompt at the top of the prompt (0: none) */
    int32_t n_keep;         /* falcon_main's --keep as given (negative: the whole prompt) */
    int32_t prompt_size;    /* tokens of the prompt, the system tokens included */
} falcon_hip_swap_cfg;
int   falcon_hip_swap_plan(const falcon_hip_swap_cfg * cfg, int n_history, int n_pending, int * n_past_new, int * n_regen);
int   falcon_hip_swap_history(const int32_t * prompt, int n_prompt, int n_batch, int32_t * history_out);
int   falcon_hip_context_set_context_stop(falcon_hip_context * c, int on);
int   falcon_hip_context_resume(falcon_hip_context * c, int seq);
int   falcon_hip_context_swap(falcon_hip_context * c, int seq, int n_past_new, const int32_t * regen, int n_regen, int n_batch);

/* ---- GUIDANCE: classifier-free guidance, a negative prompt per sequence (Sanchez et al. 2023, "Stay on topic with Classifier-Free
 * Guidance"; the arithmetic and its pinned summation order are csrc/fq_guide.h's, the operator ggml_hip_guide_rows in ggml-hip-ops.h).
 * A lock-step context evaluates the prompt's row and the negative prompt's row in one pass over the weights, each with the bits it
 * would have in a context of its own; what guidance adds sits behind lm_head and never needs the logits on the host.
 * falcon_hip_context_set_guidance(c, seq, guide_seq, scale): sequence seq (the leader) draws from
 *     log P(w | guide_seq's cache) + scale * (log P(w | seq's cache) - log P(w | guide_seq's cache))
 * in place of its logits row, with its whole sampler chain behind that (logit bias, penalties, grammar, greedy / top-k / top-p /
 * tail-free / typical / mirostat, stops, stop strings); guide_seq draws nothing -- its sampling parameters, window, generator, stops
 * and grammar are neither read nor moved -- and is FED ITS LEADER'S TOKEN: next token, position, output column and step counter move
 * with the leader's, and a leader that has ended (stops, budget, stop string) leaves its guide frozen with it, so that clearing the
 * stops continues the pair exactly. guide_seq -1 takes seq's pair apart. The caller puts the two prompts into the two slots
 * (falcon_hip_context_copy_seq, or falcon_hip_eval_seqs) at their own positions: the rows are ragged like any others.
 * falcon_hip_sample after falcon_hip_eval_seqs, and falcon_hip_decode_sample_seqs, honour the pairs; with
 * falcon_hip_context_use_graph the step stays one replay. Turning the first pair of a context on or the last off re-captures its
 * sampled step once; another pair or scale does not (device data). The loop's early exit counts a guide as ending with its leader:
 * a context in which every DRAWING sequence has stops still ends early. A guide's column of out_tokens equals its leader's, the -1
 * entries behind the end included. falcon_hip_get_logits, falcon_hip_eval_score and the log-probability records keep meaning the RAW
 * rows: a leader's record is of its raw row, a guide's record is unspecified.
 * Returns 0, or 1 after a message with nothing changed, the context usable: a context of one sequence (falcon_hip_context_create);
 * a context without lm_head; seq == guide_seq; either out of range; a guide_seq that leads or guides another sequence; a seq that
 * is itself a guide; a scale that is NaN or +-inf; the context stop on. While a pair exists falcon_hip_context_set_context_stop(on)
 * is refused, and falcon_hip_context_swap of a leader or a guide.
 * falcon_hip_context_get_guidance: guide_seq_out / scale_out [n_seq] (either may be NULL): -1 and 1 for a sequence without a guide.
 * Not covered: plain contexts, pipeline stages, the link-time wrap, draft-and-verify decode (plain contexts only), the argmax loops
 * (falcon_hip_decode_greedy_seqs ignores guidance as it ignores stops: greedy guided generation is the sampled loop at temp <= 0),
 * falcon_hip_context_copy_sampling, session files and state blobs (a binding belongs to a pair of slots and is not carried), rows
 * with logits that are not finite.                                                                                                */
int   falcon_hip_context_set_guidance(falcon_hip_context * c, int seq, int guide_seq, float scale);
int   falcon_hip_context_get_guidance(falcon_hip_context * c, int32_t * guide_seq_out, float * scale_out);

/* ---- SESSIONS: a sequence's state in the reference's own format -- llama_save_session_file / llama_load_session_file and the blob of
 * falcon_copy_state_data / falcon_set_state_data (libfalcon.cpp:4185-4564; csrc/fq_session.h restates the layout). A file written here is
 * the bytes the reference writes for the same evaluation in reference orders 1 and 2 (ggml_hip_reference_order), either side loads the
 * other's file and continues token for token. What the state holds: the generator (std::mt19937's text), the logits the last eval left on
 * the host, and K / V rows [0, n_tokens) of every layer (V transposed, as the reference keeps it; csrc/kernels_session.hip).
 * NOT in the file, because the reference does not put it there: the penalty window, mirostat's mu, stops and stop strings, grammars and their
 * states, log-probability records. The caller re-creates them from the returned tokens (set_sampling with history = the tokens, as falcon_main does from
 * session_tokens).
 * falcon_hip_session_hparams: the file's hparams record, the nine int32 of falcon_hparams in the reference's order; a load compares it
 * byte for byte with the caller's. n_ctx is the CONTEXT's n_ctx (a session only loads into a context of the length it was saved from: the
 * reference's rule, and its kv_size field follows n_ctx as well). falcon_hip_session_hparams_ggcc fills it from a GGCC file (host only;
 * 0, or -1); a model built through falcon_hip_model_set_tensor has no file: its caller fills the record.
 * falcon_hip_state_size: the bytes falcon_hip_copy_state writes for n_tokens rows (exact, not a bound; 0 for n_tokens outside 0..n_ctx).
 * logits_all: the logits section's capacity is n_ctx * n_vocab instead of n_vocab (a reference context made with logits_all).
 * falcon_hip_copy_state: sequence seq's state into dst. Logits: what the last falcon_hip_eval / eval_token left on the host -- n_vocab
 * floats, or N * n_vocab after an eval with logits_all when the capacity holds them (else its last row); falcon_hip_eval_seqs: the
 * sequence's row; size 0 when the last call was a decode loop or falcon_hip_eval_score, which leave none. Generator: the sequence's
 * sampler row if the context has one, else the generator an earlier load left for it, else std::mt19937(1).
 * falcon_hip_set_state: the rows into slot seq (no row at or beyond n_tokens, no other slot), the logits into the buffer
 * falcon_hip_get_logits returns (single-sequence contexts; their last row also onto the device, where falcon_hip_sample draws from it), the
 * generator into the sequence's sampler row if it exists -- otherwise it is kept, and the next falcon_hip_context_set_sampling[_ext] of
 * that sequence takes it over instead of seeding. n_tokens_out: the rows restored (kv_ntok).
 * Embedding: while FALCON_HIP_EMBED_LAST is set the blob holds the kept row (n_embd floats; zeros before the first eval) and is 4 * n_embd bytes
 * larger, and a load puts the row back, so that falcon_hip_get_embeddings returns it without an eval. The reference asserts that the section's size is
 * its context's, so a blob with the row loads only while the mode is set and one without it only while it is clear (code 7 otherwise).
 * falcon_hip_session_save / _load: the file around the blob -- magic, version, the record, the tokens. load: tokens_out [capacity].
 * All of them wait for the library stream, allocate their staging buffer for the call and free it after (a context that never saves keeps
 * its footprint), move no buffer of the context (captured steps stay valid: falcon_hip_context_graph_captures does not move across a
 * load) and launch nothing else: with no session call made every loop launches what it launched before.
 * Return 0 or a code, and a refused call leaves context, outputs and file as they were:                                               */
enum {
    FALCON_HIP_SESSION_E_MAGIC = 1,        /* not a session file of version 1                                                      */
    FALCON_HIP_SESSION_E_HPARAMS = 2,      /* the file's hparams record differs from the caller's                                  */
    FALCON_HIP_SESSION_E_CAPACITY = 3,     /* more tokens than tokens_out holds                                                    */
    FALCON_HIP_SESSION_E_TRUNCATED = 4,    /* shorter than its own fields say                                                      */
    FALCON_HIP_SESSION_E_NTOK = 5,         /* kv_ntok < 0 or above the context's n_ctx                                             */
    FALCON_HIP_SESSION_E_KV_SIZE = 6,      /* kv_size is not that of this model at this n_ctx                                      */
    FALCON_HIP_SESSION_E_EMBEDDING = 7,    /* the embedding section is not what this context keeps: n_embd floats with FALCON_HIP_EMBED_LAST set, else none */
    FALCON_HIP_SESSION_E_RNG = 8,          /* the generator text is not 624 words and a position in 0..624                         */
    FALCON_HIP_SESSION_E_LOGITS = 9,       /* logits size above its capacity                                                       */
    FALCON_HIP_SESSION_E_ARG = 16,         /* NULL argument, n_tokens outside 0..n_ctx                                             */
    FALCON_HIP_SESSION_E_STAGE = 17,       /* a pipeline stage (layer_begin > 0 or no lm_head): a session spans all layers         */
    FALCON_HIP_SESSION_E_SEQ = 18,         /* seq outside the context's sequences                                                  */
    FALCON_HIP_SESSION_E_CAPTURE = 19,     /* called while the library stream is capturing                                         */
    FALCON_HIP_SESSION_E_ALLOC = 20,       /* the staging buffer could not be allocated                                            */
    FALCON_HIP_SESSION_E_IO = 21           /* the file cannot be read or written                                                   */
};
typedef struct falcon_hip_session_hparams {
    int32_t n_vocab, n_ctx, n_embd, n_head, n_head_kv, n_layer, n_falcon_type, n_bpe_merges, ftype;
} falcon_hip_session_hparams;
int    falcon_hip_session_hparams_ggcc(const char * path, int n_ctx, falcon_hip_session_hparams * out);
size_t falcon_hip_state_size(const falcon_hip_context * c, int n_tokens, int logits_all);
int    falcon_hip_copy_state(falcon_hip_context * c, int seq, int n_tokens, int logits_all, void * dst);
int    falcon_hip_set_state(falcon_hip_context * c, int seq, const void * src, size_t n_bytes, int * n_tokens_out);
int    falcon_hip_session_save(falcon_hip_context * c, int seq, const char * path, const falcon_hip_session_hparams * hparams,
                               const int32_t * tokens, int n_tokens, int logits_all);
int    falcon_hip_session_load(falcon_hip_context * c, int seq, const char * path, const falcon_hip_session_hparams * hparams,
                               int32_t * tokens_out, int capacity, int * n_out);

/* ---- LoRA ADAPTERS: llama_apply_lora_from_file (libfalcon.h:187-191, libfalcon.cpp:3927-4170) on the device-resident weights. path_lora is
 * a 'ggla' file (csrc/fq_lora.h restates the format): every NAME.loraA [r, K] / NAME.loraB [r, M] pair patches the model's matrix NAME, in file
 * order, with the bits the reference's scalar build gives it: ba[m][k] = (float) sum_i (double)(float)(A[k][i] * B[m][i]), i ascending;
 * ba *= alpha / r unless that is exactly 1; a quantized matrix becomes quantize_row(dequantize_row(W) + ba), an F16 matrix fp16(fp32(W) + ba).
 * loraA may be F16 with an F32 loraB (B is then rounded to fp16 first, as ggml's f16 mat-mul does); loraB is always F32.
 * path_base_model (NULL: none): a GGCC v10 file whose F16 or F32 tensor NAME takes the place of dequantize_row(W) (--lora-base); an F16 base is
 * summed in fp16 before it is quantized, as the reference does. Quantized destinations only: an F16 matrix with a base file is refused.
 * The merge runs on the device in chunks of rows (256 MB of f32 staging; FALCON_HIP_LORA_ROWS=n: n rows per chunk, read per call), waits for
 * the device before its first write and after its last, and keeps every matrix where and how large it is: contexts of the model, their KV caches
 * and their captured steps stay valid and see the patched weights from their next call on. On a pipeline stage, matrices of other stages are
 * skipped. The whole adapter is read and checked first: a call that returns non-zero (one line on stderr) has changed nothing.
 * falcon_hip_lora_scan is the host-only part (no device needed): the checks of the file against hparams; on 0 it gives r, alpha and the
 * number of pairs. falcon_hip_model_get_tensor: the bytes of a matrix this model holds, in ggml's block layout (what the model file holds for it;
 * F16: the fp16 rows) -- dst NULL: returns the size; else copies it (cap >= size) and returns the size; -1 after a message.
 * The link-time wrap still refuses llama_apply_lora_from_file for a device context: a host that wants adapters calls this on the model.   */
enum {
    FALCON_HIP_LORA_E_IO = 1,              /* the adapter cannot be read                                                           */
    FALCON_HIP_LORA_E_MAGIC = 2,           /* bad file magic                                                                       */
    FALCON_HIP_LORA_E_VERSION = 3,         /* a version other than 1                                                               */
    FALCON_HIP_LORA_E_RANK = 4,            /* r <= 0                                                                               */
    FALCON_HIP_LORA_E_TRUNCATED = 5,       /* the header, a record or its data runs past the end of the file                       */
    FALCON_HIP_LORA_E_NOT_LORA = 6,        /* a name that does not end in .loraA / .loraB                                          */
    FALCON_HIP_LORA_E_UNKNOWN = 7,         /* a name that is not a 2-D matrix of this model                                        */
    FALCON_HIP_LORA_E_NDIMS = 8,           /* n_dims != 2                                                                          */
    FALCON_HIP_LORA_E_FTYPE = 9,           /* a data type other than F32 (0) and F16 (1)                                           */
    FALCON_HIP_LORA_E_SHAPE = 10,          /* K != loraA.ne[1] or M != loraB.ne[1]                                                 */
    FALCON_HIP_LORA_E_INNER = 11,          /* loraA.ne[0] != loraB.ne[0]                                                           */
    FALCON_HIP_LORA_E_UNPAIRED = 12,       /* a half without its other half                                                        */
    FALCON_HIP_LORA_E_TYPE_PAIR = 13,      /* a type pair other than (F32, F32) and (F16 loraA, F32 loraB)                         */
    FALCON_HIP_LORA_E_ARG = 32,            /* NULL argument                                                                        */
    FALCON_HIP_LORA_E_ROW_SPLIT = 33,      /* a matrix of a row-split (tensor-parallel) model                                      */
    FALCON_HIP_LORA_E_BASE_OPEN = 34,      /* the base model file is no readable GGCC v10 file                                     */
    FALCON_HIP_LORA_E_BASE_TENSOR = 35,    /* the base file lacks the tensor, or holds it in another shape or a quantized type     */
    FALCON_HIP_LORA_E_BASE_F16_DST = 36,   /* a base file with an F16 destination matrix                                           */
    FALCON_HIP_LORA_E_CAPTURE = 37,        /* called while the library stream is capturing                                         */
    FALCON_HIP_LORA_E_ALLOC = 38           /* the staging buffers could not be allocated                                           */
};
int     falcon_hip_model_apply_lora(falcon_hip_model * m, const char * path_lora, const char * path_base_model);
int     falcon_hip_lora_scan(const char * path, const falcon_hip_hparams * hp, int * r_out, int * alpha_out, int * n_tensors_out);
int64_t falcon_hip_model_get_tensor(falcon_hip_model * m, const char * name, void * dst, size_t cap);

/* ---- DRAFT-AND-VERIFY DECODE (csrc/fq_spec.h): the pending token and n_draft guessed continuations in ONE pass over the weights, and as
 * many of them kept as the sampler itself draws. Exact, with no rejection sampling: the pass's last launch runs the context's own sampler
 * over the n_draft + 1 logits rows in order (one generator, one window, one stop state) and stops at the first draw that is not the next
 * row's draft. Wherever a row's logits equal the single-token step's -- ggml_hip_reference_order 1 and 2 for every n_draft; the default order
 * for n_draft <= 3 on the legacy formats (the column mat-vec launches of a lock-step context of as many sequences) -- tokens, generator,
 * window, mu, stop state are those of falcon_hip_decode_sample, bit for bit; elsewhere every draw is the sampler's draw from the logits
 * falcon_hip_eval(..., logits_all) gives for the same rows. A wrong draft costs a row of a pass, never a token.
 * Plain single-sequence contexts with the whole model in one process. The rows of a pass are consecutive positions of the one cache; a
 * rejected row's K / V stay behind as stale rows at or beyond the next pass's first position, where that pass overwrites them before
 * anything reads them.
 * set_spec: n_draft 0 turns it off, 1..15 on. source GGML_HIP_SPEC_LOOKUP: prompt lookup (ggml_hip_draft_lookup's rule with ngram_min ..
 * ngram_max) over history [n_history] = every token of the sequence so far, the last one the pending token falcon_hip_decode_spec is then
 * called with; the launch appends its draws. GGML_HIP_SPEC_GIVEN: the caller's guess (set_spec_guess); history and n-grams are ignored.
 * Allocates on the first call (outside any capture) and resets the counters; the captured pass stays while n_draft, the source and the n-gram
 * bounds stay (a new history costs no capture), and n_draft 0 drops it. After falcon_hip_context_swap, a
 * falcon_hip_decode_sample or an eval that moved the sequence, give the history again -- a stale history makes worse drafts, never other tokens.
 * Returns 1 after a message, with nothing changed, for: a lock-step context, a pipeline stage, n_draft outside 0..15, n_draft + 1 >
 * n_batch, an unknown source, bad n-gram bounds, a history longer than n_ctx or with ids outside the vocabulary, and while log-probability
 * records are on (a verify pass records none; falcon_hip_context_set_logprobs(n_top >= 0) is refused likewise while spec is on).
 * set_spec_guess: tokens [n] guess the next draws, tokens[i] draw number i counted from this call (-1: no guess there); n <= n_ctx.
 * decode_spec: first_token at n_past, then passes until n_tokens draws are made or the row's stops end it. out_tokens [n_tokens]: the draws,
 * -1 behind them; *n_out their number. The count is enforced on the device (a pass never draws or writes one more), and the loop polls the
 * device every falcon_hip_context_set_stop_poll passes as the sampled loops do: at most two intervals of passes are launched past the end,
 * and they draw nothing. n_past + n_tokens <= n_ctx, unless the context stop is on: then the row ends with GGML_HIP_STOP_CONTEXT at the draw
 * that fills its cache, no position >= n_ctx is evaluated or written, and the slots behind read -1. Replays one captured pass when
 * falcon_hip_context_use_graph is on. falcon_hip_decode_sample on a context with spec on stays the plain loop. 0, 1 refused, 3 as eval.
 * get_spec_stats: since the last set_spec: passes that drew, their draws, hist_out [16]: hist_out[d - 1] = passes that made d draws.     */
int     falcon_hip_context_set_spec(falcon_hip_context * c, int n_draft, int source, int ngram_min, int ngram_max, const int32_t * history, int n_history);
int     falcon_hip_context_set_spec_guess(falcon_hip_context * c, const int32_t * tokens, int n);
int     falcon_hip_decode_spec(falcon_hip_context * c, int32_t first_token, int n_past, int n_tokens, int32_t * out_tokens, int * n_out);
int     falcon_hip_context_get_spec_stats(falcon_hip_context * c, int64_t * passes_out, int64_t * draws_out, int64_t * hist_out);

#ifdef __cplusplus
}
#endif
#endif
