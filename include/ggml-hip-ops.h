/*
 * ggml-hip-ops.h -- C ABI of libggml_hip.so, operator level. Plain pointers and sizes only.
 *
 * Each entry point names the reference operator it replaces (file:line in cmp-nct/ggllm.cpp). Pointers called
 * *_dev are device (HBM) addresses obtained from ggml_hip_malloc; everything runs on the library's stream
 * (ggml_hip_stream) unless stated. Errors are fatal (message + exit(1)), the reference backend's convention
 * (CUDA_CHECK, ggml-cuda.cu:22-51). There is NO CPU fallback: without a HIP device every call aborts.
 */
#ifndef GGML_HIP_OPS_H
#define GGML_HIP_OPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ggml_hip_weight ggml_hip_weight;   /* a weight matrix resident in HBM: quantized (re-tiled) or F16 (as in the file) */
typedef struct ggml_hip_acts   ggml_hip_acts;     /* quantized activations (Q8_0 / Q8_1 / Q8_K) in HBM      */

/* ---- device / memory plumbing (reference: ggml_init_cublas ggml-cuda.cu:1982-2041, pool 1738-1853) ---- */
int     ggml_hip_init(int device);                /* idempotent; returns number of visible HIP devices        */
int     ggml_hip_device_count(void);
/* tuning aid: wall_clock64 phase stamps (8 per workgroup) of the last k_gemv_ln [0,4096) and k_gemv_out [4096,8192) */
void    ggml_hip_debug_stamps(int enable, long long * out_host);
void    ggml_hip_debug_force_gemv(int on);        /* tests: N > 4 through column-chunked mat-vec instead of the MFMA GEMM */
void    ggml_hip_debug_ring_general(int on);      /* tests: the ring-form decode launch through its general instantiation for every shape (same bits) */
void    ggml_hip_debug_attention_form(int form);  /* tests / tuning: the prefill attention kernel for N >= 32 tokens -- 0 default (k_attention_flash: 32-token tiles, K.Q twice,
                                                     fp16 probabilities in LDS, while they fit; else 32), 1 the same forced, 32 the scratch form (scores through HBM), 16 / 17:
                                                     16-token tiles with the score rows (f32) / the probabilities (fp16, exact) in LDS; all bit-identical (ggml.c:10911-11102, 12389-12456) */
void    ggml_hip_debug_attention_plan(int N, int H, int HKV, int D, int n_past, long long * out16);   /* tests, read-only: the plan ggml_hip_attention of this shape takes now (the process's
                                                     switches and modes; csrc/fq_attn_forms.h): family (2 one row, 3 rows in LDS, 4 rows on scratch, 5 flash, 6 / 7 forms 16 / 17, 8 the
                                                     scratch form; 0 / 1 refusals), tokens per workgroup, flash pitch, KEEP, LONG, packed, packed tiles, table, persistent, grid x, y,
                                                     block, LDS bytes, row pitch, scratch bytes, FQ_ATTN_DBG */
void    ggml_hip_debug_mul_mat_plan(const ggml_hip_weight * w, int64_t N, long long * out8);   /* tests, read-only, launches nothing: the launch key of ggml_hip_mul_mat_q_acts(w, N columns)
                                                     as the process stands (its modes and switches, this device's CUs; csrc/fq_mm_forms.h fq_mm_launch_key): family, K split S,
                                                     more than one pass, streaming form, then four facts of that form (weight stages, tiles per workgroup, loops, ragged tails) */
int     ggml_hip_debug_exp_boundary(unsigned * out_host, int cap);   /* diagnostic: (input bits << 16 | table entry) of the fp16 inputs whose exp() the in-kernel formula's f32 fast
                                                     path leaves undecided (they are looked up in csrc/fq_exp_fix.h, generated from this list); returns their number */
/* tests: out_dev[i] = routine fn of (a_dev[i], b_dev[i]) for i < n, as compiled for the device (csrc/kernels_scalar_check.hip): the shared host / device scalar
 * routines the sampler, scorer, quantizer and k-quant kernels call per element, each from its production header. a, b and out are raw bits: an f32's bits, a 16-bit
 * fp16 pattern or an integer in a uint32_t; b_dev is not read (and may be NULL) for the one-argument routines. NEGLIGIBLE_F / _D: t = a, sum = b (f32, widened to
 * double on the device for _D), result 0 / 1. *_PRODUCT: the conversion applied to a * b written inline in the call. Stream-ordered, no sync. Returns 0, or 1 with
 * nothing launched for an unknown fn, n < 0, a NULL a_dev / out_dev, or a NULL b_dev with a two-argument routine. */
enum {
    GGML_HIP_SCALAR_EXPF = 0, GGML_HIP_SCALAR_LOGF, GGML_HIP_SCALAR_LOG2F, GGML_HIP_SCALAR_POWF, GGML_HIP_SCALAR_F2I_X86,       /* csrc/fq_sample.h, fq_sample_chain.h */
    GGML_HIP_SCALAR_NEGLIGIBLE_F, GGML_HIP_SCALAR_NEGLIGIBLE_D,
    GGML_HIP_SCALAR_F2H_BITS, GGML_HIP_SCALAR_F2H, GGML_HIP_SCALAR_F32_TO_F16_BITS,                                             /* fq_device.h, fq_wquant.h, fq_f16.h */
    GGML_HIP_SCALAR_F2H_BITS_PRODUCT, GGML_HIP_SCALAR_F2H_PRODUCT, GGML_HIP_SCALAR_F32_TO_F16_BITS_PRODUCT,
    GGML_HIP_SCALAR_H2F_BITS, GGML_HIP_SCALAR_H2F, GGML_HIP_SCALAR_F16_BITS_TO_F32,                                             /* fq_device.h, fq_units.h, fq_f16.h */
    GGML_HIP_SCALAR_DOT4, GGML_HIP_SCALAR_DOT4_C_HIGH, GGML_HIP_SCALAR_DOT4_C_LOW, GGML_HIP_SCALAR_DOT4_C_MID, GGML_HIP_SCALAR_DOT4Z,   /* fq_units.h; c = 0, 0x7FFFFF00, -0x7FFFFF00, 12345 */
    GGML_HIP_SCALAR_DOT2, GGML_HIP_SCALAR_DOT2_C_HIGH, GGML_HIP_SCALAR_DOT2_C_LOW, GGML_HIP_SCALAR_DOT2_C_MID, GGML_HIP_SCALAR_DOT2Z,   /* fq_kdot.h; the same c */
    GGML_HIP_SCALAR_PACK16, GGML_HIP_SCALAR_PK_SUB16, GGML_HIP_SCALAR_MUL24,
    GGML_HIP_SCALAR_COUNT
};
int     ggml_hip_debug_scalar_eval(int fn, const uint32_t * a_dev, const uint32_t * b_dev, int64_t n, uint32_t * out_dev);
/* Prefill GEMM (N > 4): by default each row's sum over its 32-element blocks is split into S interleaved partial sums,
 * P_s = blocks s, s + S, ... added left to right, result ((P0 + P1) + P2) + P3: S = 4 for matrices with fewer than 4 x #CU
 * 32x32 tiles, S = 2 above (S times the K-parallelism; 1.1-1.5 x faster). on = 1: S = 1 always, the reference's single
 * left-to-right sum (ggml_vec_dot_q*_q8_*, scalar branch) -- legacy-format results are then bit-identical with the
 * reference's scalar build.                                                                                              */
void    ggml_hip_gemm_sequential(int on);
/* on = 1: the arithmetic ORDER of the reference's portable (SIMD-less) build everywhere: every quantized mat-mul, any N,
 * through a per-thread restatement of the scalar branches of ggml_vec_dot_q*_q8_* (csrc/fq_ref_dot.h: left-to-right block
 * sums for the legacy formats, the eight float lanes of k_quants.c:1684-1746 ... for Q3_K .. Q6_K), f64 accumulation of the
 * attention's two dot products (ggml.c:2296-2300; the default is f32 fused multiply-add chains like the reference's SIMD
 * builds), N = 1 steps through the op-by-op launch list. Prefill AND decode logits of all ten formats are then
 * bit-identical with that reference build's (tests/test_gpu_falcon.py). A parity instrument: 10-100 x slower.
 * on = 2 (round 6): the SAME association -- the same bits as on = 1 and as the reference's scalar build -- on the fast kernels wherever they have it, i.e. the legacy
 * formats (Q4_0, Q4_1, Q5_0, Q5_1, Q8_0): N = 1 steps through the fused decode launches, whose lanes leave every unit's f32 term (the reference's per-block term,
 * ggml.c:2591-2609 ...) in an LDS strip [row][block] that a wave with lane = row adds left to right (csrc/fq_ref_chain.h); batches of N >= 2 through the int8-MFMA GEMM
 * with one left-to-right sum per row (ggml_hip_gemm_sequential); attention dots in f64. The k-quants: every mat-mul column by column through k_gemv_kq_ref
 * (csrc/kernels_kqref.hip: the scalar branches' eight float lanes per super-block at wave speed: ~0.5-0.7 x the default order's decode). Falcon-7B Q4_0
 * decode: 925-930 tok/s (default order 1 005-1 020, mode 1: 40). tests/test_gpu_ref_fast.py.                                                                      */
void    ggml_hip_reference_order(int on);
int     ggml_hip_get_reference_order(void);
/* ---- row-split tensor parallelism, one process per GPU (csrc/split_tp.hip): the reference's `-ts` / GGML_BACKEND_GPU_SPLIT.
 * ggml_hip_tensor_split_rows: the row range of every device for a matrix of nrows rows, with the reference's arithmetic
 *   (ggml_cuda_set_tensor_split ggml-cuda.cu:2050-2077, ggml_cuda_transform_tensor :3044-3052); host only.
 * ggml_hip_weight_upload_rows: rows [row_low, row_high) of the ggml block bytes onto this process's device (NULL: empty range).
 * ggml_hip_mul_mat_q_split: every rank multiplies its rows, then the ranks exchange them by RCCL send/recv (in place of the
 *   host-side gather on the main device, :2779-2788); dst [N][M] is complete on every rank and bit-identical to the unsplit
 *   ggml_hip_mul_mat_q. unique_id: 128 bytes of falcon_hip_pipeline_unique_id (world == 1: NULL, no RCCL).
 * ggml_hip_mul_mat_q_split_local: all ranks' parts in one process on one device (tests).                                   */
typedef struct ggml_hip_split_comm ggml_hip_split_comm;
/* joins this process to a row-split job at the ggml-cuda.h boundary: from now on ggml_cuda_transform_tensor uploads this
 * rank's rows of GGML_BACKEND_GPU_SPLIT tensors (proportions: ggml_cuda_set_tensor_split) and their mat-muls inside
 * ggml_cuda_compute_forward exchange rows by RCCL. world <= 1 leaves / restores the default (whole matrices). Returns 0; 1 (nothing changed)
 * while split tensors uploaded under the current job are still alive. */
int     ggml_hip_split_configure(int rank, int world, const void * unique_id);
void    ggml_hip_tensor_split_rows(const float * tensor_split, int n_devices, int64_t nrows, int64_t * row_low, int64_t * row_high);
ggml_hip_weight * ggml_hip_weight_upload_rows(int type, const void * host_blocks, int64_t K, int64_t nrows, int64_t row_low, int64_t row_high);
ggml_hip_split_comm * ggml_hip_split_comm_create(int rank, int world, const void * unique_id);
void    ggml_hip_split_comm_free(ggml_hip_split_comm * c);
/* collective: 0 when every rank passed the same n bytes (the shim checks the -ts proportions with it once per job), 1 otherwise */
int     ggml_hip_split_comm_agree(ggml_hip_split_comm * c, const void * bytes, size_t n);
int     ggml_hip_mul_mat_q_split(ggml_hip_split_comm * c, const ggml_hip_weight * w_rows, const float * x_dev, int64_t K, int64_t N,
                                 float * dst_dev, int64_t M, const int64_t * row_low, const int64_t * row_high);
int     ggml_hip_mul_mat_q_split_local(ggml_hip_weight * const * parts, int world, const float * x_dev, int64_t K, int64_t N,
                                       float * dst_dev, int64_t M, const int64_t * row_low, const int64_t * row_high);
/* the local form with the EXCHANGE of ggml_hip_mul_mat_q_split run for real: a communicator of one RCCL rank (this process and GPU)
 * standing for `world` virtual ranks; every part's rows are computed into a private buffer, packed, sent with a grouped ncclSend /
 * ncclRecv addressed to rank 0 itself, and unpacked into dst -- pack, RCCL calls and unpack of a real job on a single-GPU box.
 * ggml_hip_split_comm_create_loopback: NULL when RCCL is missing or refuses; ggml_hip_split_comm_rccl_ranks: ncclCommCount (0: no RCCL communicator). */
ggml_hip_split_comm * ggml_hip_split_comm_create_loopback(int virtual_world);
int     ggml_hip_split_comm_rccl_ranks(ggml_hip_split_comm * c);
int     ggml_hip_mul_mat_q_split_loopback(ggml_hip_split_comm * c, ggml_hip_weight * const * parts, const float * x_dev, int64_t K, int64_t N,
                                          float * dst_dev, int64_t M, const int64_t * row_low, const int64_t * row_high);
/* staging-buffer pool of the ggml-cuda.h boundary (ggml_cuda_compute_forward's src1 / dst device copies; the reference's
 * ggml_cuda_pool_malloc, ggml-cuda.cu:1738-1816): buffers ever allocated, hand-outs served by reuse, buffers free now */
void    ggml_hip_shim_pool_stats(size_t * n_alloc, size_t * n_reuse, size_t * n_free);
int     ggml_hip_selftest(void);                  /* device self-checks (wave reductions); 0 = pass                */
/* soft_max's fp16 EXP table entries are recomputed in the attention kernels instead of gathered when -- checked at init, for
 * every non-NaN fp16 input -- the recomputation equals the host-built table. Returns the number of mismatching inputs (0 = in
 * use), -1 when GGML_HIP_EXP_TABLE=1 forces the gather. */
int     ggml_hip_exp_formula_mismatches(void);
void *  ggml_hip_stream(void);                    /* hipStream_t used for every launch of this library        */
void *  ggml_hip_malloc(size_t bytes);
void    ggml_hip_free(void * dev);
void    ggml_hip_memcpy_h2d(void * dst_dev, const void * src_host, size_t bytes);   /* stream-ordered, then waits */
void    ggml_hip_memcpy_d2h(void * dst_host, const void * src_dev, size_t bytes);   /* stream-ordered, then waits */
void    ggml_hip_memcpy_d2d(void * dst_dev, const void * src_dev, size_t bytes);    /* stream-ordered, async      */
void    ggml_hip_memset(void * dst_dev, int value, size_t bytes);
void    ggml_hip_synchronize(void);
/* timing on the library's stream (hipEvent); elapsed in milliseconds */
void *  ggml_hip_event_create(void);
void    ggml_hip_event_record(void * ev);
float   ggml_hip_event_elapsed_ms(void * ev_start, void * ev_stop);   /* synchronises on ev_stop */
void    ggml_hip_event_destroy(void * ev);
/* per-launch timing of the quantized mat-vec kernels (hipEvents on the launch stream) for the roofline report:
 * between begin and end every GEMV launch is bracketed; end returns #launches, summed microseconds and summed
 * algorithmic bytes (the weight matrix of each launch, read once)                                            */
void    ggml_hip_profile_begin(void);
void    ggml_hip_profile_end(int64_t * n_launches, double * total_us, double * total_bytes);
double  ggml_hip_profile_bracket_overhead_us(void);   /* duration an EMPTY event bracket reports on this stream */
const uint16_t * ggml_hip_gelu_table_dev(void);   /* 65536 fp16 entries, built like ggml.c:4276-4290 */
const uint16_t * ggml_hip_exp_table_dev(void);

/* ---- weights: ggml_cuda_transform_tensor (ggml-cuda.cu:3030-3073) ---------------------------------------- */
/* host_blocks: M rows of K/blck ggml blocks exactly as in a model file (type = enum ggml_type value).
 * type 1 (GGML_TYPE_F16): M rows of K fp16 values, row-major; they stay 2 bytes per weight on the device, K must be a
 * multiple of 32 (anything else is refused: message, exit).                                                     */
ggml_hip_weight * ggml_hip_weight_upload(int type, const void * host_blocks, int64_t K, int64_t M);
void    ggml_hip_weight_free(ggml_hip_weight * w);                 /* ggml_cuda_free_data, ggml-cuda.cu:3075-3092 */
size_t  ggml_hip_weight_nbytes(const ggml_hip_weight * w);         /* == ggml_nbytes of the tensor (F16: 2 K M)  */

/* dequantize_row_q* (ggml.c:1509-1619, k_quants.c:344-876) / ggml_compute_forward_get_rows_q (ggml.c:11975):
 * dst_dev[i][0..K) = dequantized weight row rows_dev[i] (rows_dev == NULL: rows 0..nrows-1); an F16 matrix
 * (ggml_compute_forward_get_rows_f16, ggml.c:11937) is widened exactly                                         */
void    ggml_hip_dequantize_rows(const ggml_hip_weight * w, const int32_t * rows_dev, int64_t nrows, float * dst_dev);   /* rows may repeat, in any order; dst is [nrows][K], contiguous */

/* ---- weight quantizers: ggml_quantize_chunk (ggml.c:19479-19560) over quantize_row_q*_reference
 * (ggml.c:927-1129; k_quants.c:275-343, 396-471, 542-606, 652-733, 781-844) ------------------------------- */
/* nrows rows of K f32 -> nrows * K/blck ggml blocks, byte-identical with the reference's model files.
 * hist_dev: 16 int64 counters that are ADDED to (the reference's quantize histogram; legacy formats only, the
 * k-quants never count), or NULL. Returns 0, or -1 (message on stderr) for a bad type / row length.             */
int     ggml_hip_quantize_rows(int type, const float * x_dev, int64_t K, int64_t nrows, void * blocks_dev, int64_t * hist_dev);
/* same, straight into a resident weight matrix (quantize + re-tile on the device)                              */
ggml_hip_weight * ggml_hip_weight_quantize(int type, const float * x_dev, int64_t K, int64_t M);
void    ggml_hip_fp16_to_fp32_row(const uint16_t * src_dev, float * dst_dev, int64_t n);   /* ggml.c:370-374 */

/* ---- activations: INIT phase of mul_mat_q (ggml.c:11462-11476) ------------------------------------------- */
/* act_type: 8 = Q8_0 (ggml.c:1106-1129), 9 = Q8_1 (ggml.c:1292-1325), 15 = Q8_K (k_quants.c:899-934)          */
ggml_hip_acts * ggml_hip_acts_alloc(int act_type, int64_t K, int64_t max_cols);
void    ggml_hip_acts_free(ggml_hip_acts * a);
/* column c of x starts at x_dev + c * ldx: ldx >= K and a multiple of 4, x_dev 16-byte aligned (the quantizers load float4); what lies between the
 * columns is never read into a block. Columns [0, ncols) of the set are rewritten, the columns beyond keep what they held.                       */
void    ggml_hip_quantize_acts(ggml_hip_acts * a, const float * x_dev, int64_t ldx, int64_t ncols);
/* writes ncols * K/blck ggml blocks (block_q8_0 / block_q8_1 / block_q8_K bytes) for bit-exact comparison     */
void    ggml_hip_acts_export(const ggml_hip_acts * a, int64_t ncols, void * out_dev);

/* ---- quantized mat-mul: ggml_compute_forward_mul_mat_q_f32 (ggml.c:11318-11529) --------------------------- */
/* dst_dev[n*ldd + m] = sum_k W[m][k] * x[n][k] for n < N, m < M with the reference CPU arithmetic
 * (activations quantized to the weight type's vec_dot_type, exact integer block dots, f32 epilogue).          */
/* Strides and extents of the quantized formats, here and in ggml_hip_mul_mat_q_acts (held per kernel form by tests/test_gpu_op_contract.py): ldx as for ggml_hip_quantize_acts; ldd any
 * value >= M, odd ones included. Exactly the N * M words dst_dev[n*ldd + m] are written -- nothing between the columns, in front of column 0 or behind
 * column N - 1, whatever tile a kernel rounds M and N up to -- and rows from one 32-element block (K = 32), one super-block (K = 256 for the k-quants) and
 * one row (M = 1) on are served.                                                                                                                 */
void    ggml_hip_mul_mat_q(const ggml_hip_weight * w, const float * x_dev, int64_t ldx, int64_t N,
                           float * dst_dev, int64_t ldd);
/* ---- F16 mat-mul: ggml_compute_forward_mul_mat_f16_f32 (ggml.c:11104-11316) over ggml_vec_dot_f16 (ggml.c:2306-2340) -------
 * w: a weight uploaded with type 1. Every column of x is rounded to fp16 (round to nearest even, subnormals kept; finite
 * inputs up to 65504 in magnitude), then dst_dev[n*ldd + m] = (float) sum, sum a DOUBLE that starts at 0 and takes
 * (double)((float) W[m][k] * (float) x16[n][k]) for k = 0 .. K-1 in that order: the reference's scalar build, bit for bit
 * (csrc/fq_f16.h, csrc/kernels_f16.hip). The result of a column does not depend on N, and ggml_hip_reference_order does not
 * change it: there is one order. ggml_hip_mul_mat_q forwards F16 weights here.                                              */
void    ggml_hip_mul_mat_f16(const ggml_hip_weight * w, const float * x_dev, int64_t ldx, int64_t N,
                             float * dst_dev, int64_t ldd);
/* same, activations already quantized; epilogue: 0 = store, 1 = GELU (ggml.c:3477-3484: the fp16 table entry of the value rounded to fp16),
 * 2 = dst[n*ldd + m] = (v + add1[n*ldd + m]) + add2[n*ldd + m] (libfalcon.cpp:2399-2400): add1 and add2 are [N][M] at the SAME column stride ldd as dst and
 * are read at those N * M elements only; dst may be add2 itself (the residual stream updated in place), never add1 and never a partial overlap.
 * Epilogues 0 and 1 ignore add1 / add2 (NULL).                                                                                                  */
void    ggml_hip_mul_mat_q_acts(const ggml_hip_weight * w, const ggml_hip_acts * a, int64_t N, float * dst_dev,
                                int64_t ldd, int epilogue, const float * add1_dev, const float * add2_dev);

/* ---- the other ops of a Falcon block ------------------------------------------------------------------------ */
/* ggml_norm (ggml.c:10540-10594) followed by * w + b (libfalcon.cpp:2166-2188); w_dev == NULL: plain norm       */
/* rows of n contiguous floats; n a multiple of 4 and at most 40944 (a row and its reduction space live in the CU's 160 KiB of LDS), x_dev / w_dev / b_dev /
 * y_dev 16-byte aligned. Any other n: a message on stderr, nothing launched, y untouched.                                                      */
void    ggml_hip_layer_norm(const float * x_dev, int64_t n, int64_t rows, const float * w_dev, const float * b_dev, float * y_dev);
void    ggml_hip_gelu(const float * x_dev, float * y_dev, int64_t n);                 /* ggml.c:3477-3484 */
void    ggml_hip_add3(const float * a, const float * b, const float * c, float * y, int64_t n);   /* (a+b)+c */
/* cos/sin table for ggml_rope mode 2 with Falcon's dynamic-NTK flags (ggml.c:12875-12898, libfalcon.cpp:2229-2234):
 * returns a device table [n_pos][head_dim/2][2]                                                                */
float * ggml_hip_rope_table_create(int head_dim, int n_pos, int rope_n_ctx);
/* rotate Q in place, rotate K into k_cache, copy V into v_cache at positions n_past..n_past+N-1
 * (ggml.c:12957-12978, libfalcon.cpp:2238-2280). qkv_dev rows are [H q-heads | HKV k-heads | HKV v-heads] x D. */
void    ggml_hip_rope_kv_store(float * qkv_dev, int N, int H, int HKV, int D, int n_past, const float * rope_table_dev,
                               float * k_cache_dev, float * v_cache_dev);
/* K.Q, scale 1/sqrt(D), causal mask, soft_max, V.P, merge heads (libfalcon.cpp:2285-2366):
 * att_dev[N][H*D]; caches are [n_ctx][HKV][D] f32 for ONE layer                                                */
void    ggml_hip_attention(const float * qkv_dev, int N, int H, int HKV, int D, int n_past,
                           const float * k_cache_dev, const float * v_cache_dev, float * att_dev);
/* tests / tuning: the decode step's stand-alone attention launch for n_seq rows of one token each -- q and the new key rotated, key / value appended at the row's
 * position, attention over keys [0, pos], optionally the Q8_0 / Q8_1 image of the output rows (att_image: a ggml_hip_acts of H*64 values, >= n_seq columns).
 * qkv_dev [n_seq][(H + 2 HKV) * 64] unrotated; pos_stride 0: every row at pos_dev[0], 1: row t at pos_dev[t]; max_n_kv > every position sizes the score row and
 * bounds the early loads (both caches hold max_n_kv rows per sequence, seq_stride floats apart; rope_table_dev covers at least max_n_kv positions; no
 * pointer but att_dev / att_image may be NULL -- a test entry, it does not check them). n_seq == 1 && pos_stride == 0: k_attn_decode (k_attn_decode_f64
 * under ggml_hip_reference_order), else k_attn_decode_seqs. A max_n_kv whose score row does not fit the LDS (> 38 704) is refused: message, nothing launched. */
void    ggml_hip_attention_decode(const float * qkv_dev, int n_seq, int H, int HKV, const int * pos_dev, int pos_stride, int max_n_kv,
                                  const float * rope_table_dev, float * k_cache_dev, float * v_cache_dev, int64_t seq_stride,
                                  float * att_dev, ggml_hip_acts * att_image, int att_act_type);


/* ---- sampling: falcon_main's default chain (examples/falcon/falcon_main.cpp:896-980, libfalcon.cpp:3038-3466) ------
 * logit bias, repetition / frequency / presence penalties over the last repeat_last_n tokens, then greedy (temp <= 0:
 * the first maximum) or top-k, top-p, temperature and llama_sample_token's mt19937 draw -- the same tokens and the same
 * generator stream as the reference's functions for the same logits and seed, on rows without ties among the kept
 * candidates or at the k boundary (ties: value descending, id ascending). One sampler holds n_rows independent rows
 * (parameters, window, generator) in device memory; the logits are never written.                                      */
typedef struct ggml_hip_sampling {
    float    temp;                 /* <= 0: greedy (after the penalties)                                                  */
    int32_t  top_k;                /* <= 0: the whole vocabulary                                                          */
    float    top_p;                /* >= 1: off                                                                            */
    float    repeat_penalty;       /* 1: off                                                                               */
    int32_t  repeat_last_n;        /* window length; -1: n_ctx; 0: no penalties                                            */
    float    alpha_frequency, alpha_presence;
    float    tfs_z, typical_p;     /* set_row: must be 1; honoured by set_row_ext (>= 1: off)                              */
    int32_t  mirostat;             /* set_row: must be 0; honoured by set_row_ext (1, 2)                                   */
    uint32_t seed;                 /* std::mt19937(seed), as llama_set_rng_seed                                            */
    int32_t  n_bias;               /* logit bias entries (<= 16, distinct ids): logits[bias_id[i]] += bias[i]              */
    int32_t  bias_id[16];
    float    bias[16];
} ggml_hip_sampling;
typedef struct ggml_hip_sampler ggml_hip_sampler;
/* n_vocab <= 131072; NULL on bad sizes. Rows start greedy with an empty window until set_row.                          */
ggml_hip_sampler * ggml_hip_sampler_create(int n_rows, int n_vocab, int n_ctx);
void    ggml_hip_sampler_free(ggml_hip_sampler * s);
/* the row's parameters, generator (seeded) and window: the last min(repeat_last_n, n_ctx) tokens of n_ctx zeros followed
 * by history[0..n_history) (falcon_main's last_n_tokens). Returns 0, or 1 (refused, nothing changed) for tfs_z != 1,
 * typical_p != 1, mirostat != 0, more than 16 or repeated or out-of-range bias ids, out-of-range history ids, a window of
 * more than 4096 tokens.                                                                                                  */
int     ggml_hip_sampler_set_row(ggml_hip_sampler * s, int row, const ggml_hip_sampling * params, const int32_t * history, int n_history);
/* row src_row of src (parameters, window, generator state) -> row dst_row of dst, stream-ordered: the copy continues the source's
 * stream. 0, or 1 (nothing copied) for rows out of range, different vocabularies or a window longer than dst's n_ctx.     */
int     ggml_hip_sampler_copy_row(ggml_hip_sampler * dst, int dst_row, const ggml_hip_sampler * src, int src_row);
/* stream-ordered: tokens_dev[r] = the draw from logits_dev + r * row_stride for every row r; each row's window takes the
 * token and its generator advances                                                                                        */
void    ggml_hip_sampler_sample(ggml_hip_sampler * s, const float * logits_dev, int64_t row_stride, int32_t * tokens_dev);

/* ---- the rest of falcon_main's sampling branches (falcon_main.cpp:960-981; csrc/fq_sample_chain.h): tail-free and typical
 * in the default chain (top-k, tail-free, typical, top-p, temperature, draw) and mirostat 1 (m = 100, N = the sampler's
 * n_vocab) and 2, which ignore top_k, top_p, tfs_z and typical_p as the reference does; penalties and logit bias come first
 * in every branch, temp <= 0 is greedy in every branch. The tokens and the generator stream are those of the reference's
 * functions for the same logits, seed and mu on rows where (a) no two candidates tie in logit among those kept or at a cut,
 * (b) typical's kept candidates and the first one dropped have distinct shifted scores, (c) every probability a logf / log2f
 * is taken of is a normal number; elsewhere the device follows csrc/fq_sample_chain.h's tie rule, deterministically.
 * LIMIT: tail-free and typical run on the top-k survivors in LDS, so a tfs_z < 1 or typical_p < 1 needs 1 <= top_k <= 1024
 * (unless mirostat or greedy makes them moot).
 * set_row_ext: set_row's arguments and refusals (but tfs_z / typical_p / mirostat, which it reads from base), and refuses
 * (1, a message, nothing changed) a mirostat outside 0..2, the limit above, and with mirostat 1 / 2 a tau or eta that is
 * not finite. The row's mu starts at 2 * tau (falcon_main's static); it lives in device memory, moves with every draw of a
 * mirostat row in the sampling launch itself, is frozen with a row that has ended (stops) and travels with copy_row.
 * set_row on the row turns the new stages off again. While no row uses them the sampler launches what it launched before.
 * get_mu: mu_out[n_rows]; waits for the library stream. Rows without mirostat report the value they were set with
 * (2 * tau; 0 after set_row or before any).                                                                              */
typedef struct ggml_hip_sampling_ext {
    ggml_hip_sampling base;
    float    mirostat_tau, mirostat_eta;      /* target surprise and learning rate (falcon_main: 5.0, 0.1)                */
} ggml_hip_sampling_ext;
int     ggml_hip_sampler_set_row_ext(ggml_hip_sampler * s, int row, const ggml_hip_sampling_ext * params, const int32_t * history, int n_history);
int     ggml_hip_sampler_get_mu(ggml_hip_sampler * s, float * mu_out);
/* a row's generator as std::mt19937 holds it: 624 state words and the position of the next word (624 right after seeding, when
 * the next draw twists first). get waits for the library stream; set replaces the row's generator and nothing else of the row.
 * How a saved session's generator (falcon-hip.h) reaches the row that draws. 0, or 1 (message, nothing changed) for a bad row
 * or a position outside 0..624.                                                                                             */
int     ggml_hip_sampler_get_rng(ggml_hip_sampler * s, int row, uint32_t * words_out, int32_t * pos_out);
int     ggml_hip_sampler_set_rng(ggml_hip_sampler * s, int row, const uint32_t * words, int32_t pos);

/* ---- session staging (csrc/kernels_session.hip): a sequence's K and V rows between an f32 cache [layer][row][n_head_kv * 64]
 * and a contiguous staging buffer in the reference's session-file layout (libfalcon.cpp:4271-4338):
 *   K  [n_layer][n_tok][n_head_kv * 64]   followed by   V  [n_layer][n_head_kv * 64][n_tok]   (V transposed)
 * = 2 * n_layer * n_tok * n_head_kv * 64 floats. The sequence's rows are [first_row, first_row + n_tok) of every layer; layers
 * lie layer_pitch_rows rows apart (n_ctx for a plain cache, n_seq * n_ctx for lock-step slots, where first_row = seq * n_ctx).
 * One launch each on the library stream, 64-bit offsets. pack reads the cache and writes exactly the staging floats above;
 * unpack writes exactly those cache rows (no row at or beyond n_tok, no other slot). n_tok 0: nothing is launched.
 * 0, or 1 (message, nothing launched) for NULL pointers, n_layer outside 1..65535, n_head_kv < 1, n_tok < 0, first_row < 0 or
 * layer_pitch_rows < first_row + n_tok.                                                                                      */
int     ggml_hip_kv_pack(const float * k_cache_dev, const float * v_cache_dev, float * staging_dev, int n_layer, int n_head_kv, int n_tok,
                         int64_t layer_pitch_rows, int64_t first_row);
int     ggml_hip_kv_unpack(float * k_cache_dev, float * v_cache_dev, const float * staging_dev, int n_layer, int n_head_kv, int n_tok,
                           int64_t layer_pitch_rows, int64_t first_row);

/* ---- stops (csrc/fq_stop.h): a row ends on the device. Per row up to 16 stop sequences of 1..8 token ids and a budget
 * max_tokens (0: none) of DRAWN tokens: tokens this row's sampler drew since its stops were last set (a history given to
 * set_row is not drawn). After every draw the row ends with reason k if sequence k equals its last len[k] drawn tokens (the
 * lowest such k), else with GGML_HIP_STOP_BUDGET once max_tokens tokens are drawn. A row that has ended is FROZEN: later
 * ggml_hip_sampler_sample calls draw nothing for it -- its generator, window and tokens_dev entry stay as they are -- until
 * its stops are set again. Off by default; with no stops set on any row the sampler launches what it launched before.
 * set_stops: the row's sequences and budget; n_drawn, the tail of drawn tokens and the reason start afresh (also when the
 * same stops are set again). NULL: off for the row. Neither touches the generator or the window. Returns 0, or 1 after a
 * message, with nothing changed, for a row out of range, n_seqs outside 0..16, a length outside 1..8, an id outside the
 * vocabulary or max_tokens < 0.
 * get_stops: n_drawn_out / reason_out [n_rows] (either may be NULL); rows with stops off report GGML_HIP_STOP_RUNNING and 0
 * drawn. Waits for the library stream. ggml_hip_sampler_copy_row carries a row's stops and their state (off stays off).  */
#define GGML_HIP_STOP_MAX_SEQS 16
#define GGML_HIP_STOP_MAX_LEN   8
#define GGML_HIP_STOP_RUNNING (-1)
#define GGML_HIP_STOP_BUDGET  (-2)
typedef struct ggml_hip_stops {
    int32_t n_seqs;
    int32_t len[GGML_HIP_STOP_MAX_SEQS];
    int32_t tok[GGML_HIP_STOP_MAX_SEQS][GGML_HIP_STOP_MAX_LEN];
    int32_t max_tokens;
} ggml_hip_stops;
int     ggml_hip_sampler_set_stops(ggml_hip_sampler * s, int row, const ggml_hip_stops * stops);
int     ggml_hip_sampler_get_stops(ggml_hip_sampler * s, int32_t * n_drawn_out, int32_t * reason_out);

/* ---- the end of the cache (csrc/fq_stop.h: fq_stop_context): a row ends where its KV cache is full, and can run again.
 * set_context_stop(limit): limit > 0 turns it on for the whole sampler, 0 off (the default). While on, every row has stops --
 * zero id sequences and no budget unless set_stops gave some, the way set_stop_text turns a row on -- and the model-level
 * loops, which advance a position per row, hand the limit to the launch: a draw made at position limit - 1 does NOT move the
 * row's position or its tokens_dev entry, and if no other rule ended the row at that draw it ends with
 * GGML_HIP_STOP_CONTEXT. Order on one draw: id sequences, budget, strings, then this. The drawn token has entered the window,
 * the id tail and the byte ring, is counted in n_drawn and written to the loop's output: it is the token that waits to be
 * evaluated. The frozen row evaluates the same token at the same position again; no position >= limit is evaluated.
 * ggml_hip_sampler_sample, which knows no positions, ignores the limit. Rows that had no stops start from a fresh state; rows
 * that had some keep theirs. Off: rows without id sequences, budget or strings go off again. 0, or 1 for limit < 0.
 * resume(row): a row that ended with GGML_HIP_STOP_CONTEXT runs again; nothing else changes -- not n_drawn, the id tail, the
 * byte ring, cut_bytes, the generator, the window or mirostat's mu. 0, or 1 after a message, nothing changed, for a row out
 * of range or a row whose reason is anything else. Waits for the library stream.                                          */
#define GGML_HIP_STOP_CONTEXT (-3)
int     ggml_hip_sampler_set_context_stop(ggml_hip_sampler * s, int limit);
int     ggml_hip_sampler_resume(ggml_hip_sampler * s, int row);

/* ---- stop strings (csrc/fq_stop_text.h): a row ends on the BYTES it generated, however the model spelt them in tokens. Per
 * row up to 16 stop strings of 1..32 bytes. The row's drawn text is the concatenation of the bytes of the tokens drawn since
 * its stops were last set (a history given to set_row is not drawn); a token's bytes come from the vocabulary's bytes, two
 * device arrays made by set_vocab_bytes: a pool and n_vocab + 1 offsets, token t being pool[offsets[t] .. offsets[t + 1]).
 * After a draw of a token with bytes b[0..L) the row ends if some string is a suffix of the drawn text up to and including
 * b[j]: the smallest such j wins, among the strings completing there the lowest index k. The reason (get_stops) is
 * GGML_HIP_STOP_TEXT0 + k, and cut_bytes = len[k] + (L - 1 - j) counts the bytes from the match's first byte to the end of
 * the drawn text: drop that many bytes from the end of the detokenised drawn tokens to get the text before the stop string
 * (the cut may reach into earlier tokens and into the middle of one). A string longer than the drawn text cannot match; a
 * token without bytes matches nothing; a token may be longer than 32 bytes and hold a whole match.
 * Order on one draw: the id sequences, then the budget (above), then the strings: a text match replaces RUNNING and BUDGET,
 * never an id match. The row is then frozen like any ended row.
 * set_vocab_bytes: copies pool_host (offsets_host[n_vocab] bytes) and offsets_host (n_vocab + 1 words) to the device. 0, or 1
 * after a message, with nothing changed, for offsets that do not start at 0 or do not ascend or a pool beyond 16 MB.
 * set_stop_text: the row's strings (NULL: off). Turns the row's stops on -- with zero id sequences and no budget if set_stops
 * gave none -- and starts the whole shared state afresh: n_drawn, reason, the id tail, the byte ring, cut_bytes.
 * ggml_hip_sampler_set_stops on a row with strings starts the same state afresh (NULL there: the strings stay, the row stays
 * on). 0, or 1 after a message, with nothing changed, for a row out of range, n outside 0..16, a length outside 1..32, or
 * no vocabulary bytes set. get_stop_text: cut_bytes_out [n_rows], 0 while the row has not ended by text; waits for the
 * library stream. ggml_hip_sampler_copy_row carries strings, ring and cut_bytes with the row (refused, rc 1, when the
 * destination has no vocabulary bytes). With no strings set on any row the sampler launches what it launched before.    */
#define GGML_HIP_STOP_TEXT_MAX     16
#define GGML_HIP_STOP_TEXT_MAX_LEN 32
#define GGML_HIP_STOP_TEXT0        16      /* reason of string 0: the first value an id sequence cannot produce */
typedef struct ggml_hip_stop_text {
    int32_t n;
    int32_t len[GGML_HIP_STOP_TEXT_MAX];
    uint8_t bytes[GGML_HIP_STOP_TEXT_MAX][GGML_HIP_STOP_TEXT_MAX_LEN];
} ggml_hip_stop_text;
int     ggml_hip_sampler_set_vocab_bytes(ggml_hip_sampler * s, const uint8_t * pool_host, const int32_t * offsets_host);
int     ggml_hip_sampler_set_stop_text(ggml_hip_sampler * s, int row, const ggml_hip_stop_text * text);
int     ggml_hip_sampler_get_stop_text(ggml_hip_sampler * s, int32_t * cut_bytes_out);

/* ---- draft and verify (csrc/fq_spec.h): several draws from one pass over the weights, the SAME draws. The caller evaluated the
 * pending token and n_rows - 1 guessed continuations ("drafts") in one pass: logits row j (logits_dev + j * row_stride) belongs to
 * the token at position pos + j, row 0 to the pending one, row j >= 1 to draft j.
 * ggml_hip_sampler_verify_rows runs ROW 0 OF THE SAMPLER over the logits rows in order -- bias, penalties over the window, top-k /
 * top-p / temperature / draw or the set_row_ext stages, the row's stops -- exactly as ggml_hip_sampler_sample would, one draw
 * after the other with the one generator, window, mu and stop state, and goes on from row j to row j + 1 only while the draw made
 * from row j equals drafts_dev[j] (draft j + 1; -1: no draft, never equal) and no stop rule ended the row. out_dev [n_rows] gets the
 * draws, -1 behind them; n_out_dev [1] their number (0 for a row that had ended before: nothing of it moves). Wherever a logits
 * row equals the row a single-token step would have produced, tokens and sampler state are those of as many
 * ggml_hip_sampler_sample calls, bit for bit; a wrong draft only ends the pass early. Like ggml_hip_sampler_sample it knows no
 * positions and ignores the context stop. n_rows 1..16; the sampler's other rows are not touched. Waits for the library stream.
 * ggml_hip_draft_lookup makes drafts by prompt lookup: history_dev [n] = prompt plus draws, its last token the pending one. For
 * g = ngram_max down to ngram_min, the LARGEST j <= n - g - 1 with history[j .. j+g) == history[n-g .. n); the first g that has
 * one gives drafts_out_dev[i - 1] = history[j + g + i - 1] for i = 1..n_draft, -1 where that index is >= n; no g: all -1.
 * One workgroup, one max-reduction over the history. 1 <= ngram_min <= ngram_max <= 32, n_draft 1..15. Stream-ordered, no sync.
 * Both return 0, or 1 after a message with nothing launched.                                                                   */
#define GGML_HIP_SPEC_MAX_DRAFT 15
#define GGML_HIP_SPEC_LOOKUP    1
#define GGML_HIP_SPEC_GIVEN     2
int     ggml_hip_sampler_verify_rows(ggml_hip_sampler * s, const float * logits_dev, int64_t row_stride, int n_rows,
                                     const int32_t * drafts_dev, int32_t * out_dev, int32_t * n_out_dev);
int     ggml_hip_draft_lookup(const int32_t * history_dev, int n, int ngram_min, int ngram_max, int n_draft, int32_t * drafts_out_dev);

/* ---- constrained decoding (csrc/fq_grammar.h, csrc/kernels_grammar.hip): a row draws only tokens a byte automaton allows. At every
 * draw a constrained row behaves AS IF IT HAD A -inf LOGIT BIAS ON EVERY TOKEN THE CONSTRAINT FORBIDS AT THAT POINT (the reference's
 * --logit-bias id-inf), applied behind bias and penalties; the logits are not written.
 * The automaton (ggml_hip_dfa): n_states states (1..16384), trans[n_states][256], accept[n_states], a start state. State 0 is the dead
 * state: all its transitions are 0 and it never accepts. The state after a token is the state after its bytes. Token t is allowed in
 * state s: t == eos_id (-1: none) exactly when accept[s], and drawing it leaves the state as it is; a token without bytes never; any
 * other token exactly when the walk from s over its bytes does not end in 0.
 * grammar_create: copies the vocabulary's bytes (as ggml_hip_sampler_set_vocab_bytes takes them) and the table to the device and builds
 * the index there in one launch: uint64_t allow[n_states][ceil(n_vocab / 64)], bit t % 64 of word t / 64 set exactly when t is
 * allowed, bits at and beyond n_vocab 0, state 0's row all 0 (ceil(n_vocab / 64) * 8 bytes a state). NULL after a message, with
 * nothing left behind, for: bad sizes, start state or eos_id (grammar_last_error() == GGML_HIP_GRAMMAR_BAD_ARGS); a transition
 * >= n_states or out of state 0 (BAD_TRANS, *bad_state = the state whose row holds it); a state other than 0 that allows no token
 * (DEAD_END, *bad_state = the lowest such state). bad_state may be NULL; it is -1 where no state is to blame.
 * grammar_free: 0, or 1 after a message with nothing freed while a sampler row holds the grammar. get_index: rows [state0, state0 + n)
 * of the index to out (host), for tests and tools.
 * sampler_set_grammar: row's grammar (NULL: none) and state (-1: the start state). 0, or 1 after a message with nothing changed for a
 * row or state out of range or a grammar over another n_vocab. Grammars and states are device data: setting either is no reason to
 * capture a step again, but for the first grammar on and the last off (another instantiation of the kernel). After every draw the
 * row's state is the state after the drawn token, also at the draw that ends the row by a stop rule; a row that had ended before
 * moves nothing. get_grammar_state: states_out [n_rows], -1 for rows without a grammar; waits for the library stream.
 * ggml_hip_sampler_copy_row carries binding and state. A row without a grammar draws exactly what it draws without any.
 * Not covered: ggml_hip_sampler_verify_rows (refused while row 0 holds a grammar).                                                */
#define GGML_HIP_GRAMMAR_MAX_STATES 16384
#define GGML_HIP_GRAMMAR_BAD_ARGS   1
#define GGML_HIP_GRAMMAR_BAD_TRANS  2
#define GGML_HIP_GRAMMAR_DEAD_END   3
typedef struct ggml_hip_dfa {
    int32_t n_states, start;
    const uint16_t * trans;     /* [n_states][256] */
    const uint8_t * accept;     /* [n_states] */
} ggml_hip_dfa;
typedef struct ggml_hip_grammar ggml_hip_grammar;
ggml_hip_grammar * ggml_hip_grammar_create(int n_vocab, const uint8_t * pool_host, const int32_t * offsets_host, const ggml_hip_dfa * dfa, int eos_id, int * bad_state);
int     ggml_hip_grammar_last_error(void);
int     ggml_hip_grammar_free(ggml_hip_grammar * g);
int     ggml_hip_grammar_get_index(ggml_hip_grammar * g, int state0, int n, uint64_t * out);
int     ggml_hip_sampler_set_grammar(ggml_hip_sampler * s, int row, ggml_hip_grammar * g, int state);
int     ggml_hip_sampler_get_grammar_state(ggml_hip_sampler * s, int32_t * states_out);

/* ---- scoring (csrc/kernels_score.hip, csrc/fq_score.h): prob_dev[r] = the reference's soft-max probability of token
 * targets_dev[r] in row r -- float max, float expf(l - max) as the host libm computes it, a double sum over v = 0 .. n_vocab-1
 * in that order, (float)(e_t / sum).
 * falcon_perplexity.cpp:12-27 for n_rows rows of n_vocab logits (row r at logits_dev + r * row_stride); rows with
 * targets_dev[r] < 0 are skipped (nothing written for them). max_dev / sum_dev may be NULL. Stream-ordered, no sync. */
void ggml_hip_score_rows(const float * logits_dev, int64_t row_stride, int n_rows, int n_vocab,
                         const int32_t * targets_dev, float * prob_dev, float * max_dev, double * sum_dev);

/* ---- classifier-free guidance (csrc/kernels_guide.hip, csrc/fq_guide.h; Sanchez et al. 2023): a leader row steered by a guide
 * row, the row of the same position under a negative prompt. For pair p, with x_b = logits row lead_dev[p], x_g = logits row
 * guide_dev[p] (row r at logits_dev + r * row_stride) and s = scale_dev[p]:
 *   mixed_dev[p * mixed_stride + v] = lp_g[v] + s * (lp_b[v] - lp_g[v]),   lp_r[v] = (x_r[v] - max_r) - logf((float) S_r),
 * every operation a rounded float operation (no fused multiply-add), logf the host libm's, S_r the double sum of
 * expf(x_r[v] - max_r) IN THE PINNED ORDER of csrc/fq_guide.h: 256 partial sums, groups of four consecutive elements dealt
 * round-robin to them, each summed in increasing v, then combined by the butterfly q_j += q_{j xor o}, o = 1, 2, .., 128. This is
 * NOT ggml_hip_score_rows' in-order sum: the two differ in their last bits on most rows. s = 1 gives lp_b, s = 0 lp_g.
 * One workgroup per pair; a pair's result depends on its two rows and its scale alone (not on n_pairs, its place in the launch or
 * ggml_hip_reference_order). The logits are read, never written; rows no pair names are not read. A pair with lead_dev[p] < 0 is
 * skipped: nothing is read or written for it. max_dev / sum_dev (optional): [n_pairs][2], {leader, guide}, the rows' maxima and
 * sums, for tests. Needs n_vocab >= 1 and mixed_stride >= n_vocab (else a message and exit, as score_rows). The row indices are
 * device data and are not checked. Not covered: rows that hold +-inf or NaN, a scale that is not finite. Stream-ordered, no sync.
 *
 * A sampler row may have a guide row. set_guidance(s, row, guide_row, scale) makes (row, guide_row) a pair; guide_row -1 takes
 * row's pair apart. While any pair exists, ggml_hip_sampler_sample (and the model-level sampled loops) launch the mix in front
 * of the sampler's launch on the same stream, into rows the sampler owns, and then
 *   - a leader draws from its mixed row in place of its logits row; everything behind that -- logit bias, penalties, grammar
 *     mask, greedy, top-k / top-p, tail-free / typical / mirostat, stops, stop strings -- runs on the mixed row, and the row's
 *     generator, window, stop state and grammar state advance as they always do;
 *   - a guide row draws nothing: its parameters, window, generator, stops and grammar are neither read nor moved. Its
 *     tokens_dev entry (and in the loops its position, output slot, step counter and skip word) is written by its leader, with
 *     the leader's values, exactly when the leader writes its own: a leader that has ended leaves its guide row frozen with it.
 * Pairs and scales are device data: changing them is no reason to capture a step again, but for the first pair on and the
 * last off (another kernel, one more launch). While no row has a guide row the sampler launches what it launched before.
 * set_guidance returns 0, or 1 after a message with nothing changed for: row == guide_row; either index out of range; a
 * guide_row that leads a row or guides another row; a row that is itself a guide row; a scale that is NaN or +-inf; a sampler
 * whose context stop is on (and ggml_hip_sampler_set_context_stop(limit > 0) is refused while a pair exists). A row that has a
 * guide row already gets the new one, and the old one is free again. Waits for the library stream.
 * get_guidance: guide_row_out / scale_out [n_rows] (either may be NULL): -1 and 1 for a row without a guide row.
 * Not covered: ggml_hip_sampler_verify_rows (it never sees guidance), ggml_hip_sampler_copy_row (a binding belongs to a pair
 * of slots, not to a row: it is not carried).                                                                              */
void ggml_hip_guide_rows(const float * logits_dev, int64_t row_stride, int n_vocab, int n_pairs,
                         const int32_t * lead_dev, const int32_t * guide_dev, const float * scale_dev,
                         float * mixed_dev, int64_t mixed_stride, float * max_dev, double * sum_dev);
int  ggml_hip_sampler_set_guidance(ggml_hip_sampler * s, int row, int guide_row, float scale);
int  ggml_hip_sampler_get_guidance(ggml_hip_sampler * s, int32_t * guide_row_out, float * scale_out);

/* ---- log-probabilities (csrc/kernels_logprob.hip, csrc/fq_logprob.h): per row r of n_vocab logits, prob_dev[r] = the
 * probability ggml_hip_score_rows gives token chosen_dev[r] (bit for bit: same max, same sequential double sum), and the n_top
 * most likely ids with theirs: top_id_dev[r][n_top] in the sampler's candidate order (value descending, ties by id ascending,
 * compared on the bits: +0 above -0; -inf last with probability 0) and top_prob_dev[r][n_top]. The probabilities belong to the
 * raw row: no bias, penalty, temperature or truncation. chosen_dev[r] < 0: prob_dev[r] = NaN, the top-n are still written.
 * max_dev / sum_dev may be NULL; top_* may be NULL when n_top == 0. Returns 1 after a message, with nothing launched, for
 * n_top < 0, n_top > GGML_HIP_LOGPROB_MAX_TOP, n_top > n_vocab or a missing pointer. Stream-ordered, no sync.            */
#define GGML_HIP_LOGPROB_MAX_TOP 32
int  ggml_hip_logprob_rows(const float * logits_dev, int64_t row_stride, int n_rows, int n_vocab,
                           const int32_t * chosen_dev, int n_top,
                           float * prob_dev, int32_t * top_id_dev, float * top_prob_dev,
                           float * max_dev, double * sum_dev);

/* ---- pooled text vectors (csrc/kernels_embed.hip, csrc/fq_embed.h). acc_dev: n_embd doubles, count_dev: one int64, both zeroed by the
 * caller to start a text. accum: acc[col] = acc[col] + (double) rows[i][col] for i = 0 .. n_rows-1 in that order (rows n_embd floats
 * apart), count += n_rows; calls continue one another's chains. Stream-ordered, no sync; 1 after a message for a missing pointer or size.
 * finish: out[col] = (float)(acc[col] / (double) count), or with normalize that mean divided in f64 by the square root of the f64 sum of
 * the means' squares (256 strided partial chains, combined in order: one fixed order, the same from run to run). It reads count (and
 * the sum) back, so it synchronises: 1 for count 0, 2 for a zero mean vector, 3 for a missing pointer -- a message and out_dev untouched. */
int  ggml_hip_embed_pool_accum(const float * rows_dev, int n_rows, int n_embd, double * acc_dev, int64_t * count_dev);
int  ggml_hip_embed_pool_finish(const double * acc_dev, const int64_t * count_dev, int n_embd, int normalize, float * out_dev);

#ifdef __cplusplus
}
#endif
#endif
