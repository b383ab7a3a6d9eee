// kernels_block.hip -- the non-mat-mul ops of a Falcon decoder block, device resident (gfx950).
//
// In the reference these always run on the CPU, even in its CUDA build (libfalcon.cpp:2309, 2356 set
// cuda_op_directive = 0; ggml-cuda.cu:2433 supports rope mode 0 only). Arithmetic follows the CPU ops so that
// logits match the CPU reference:
//   layer norm  ggml.c:10540-10594  (f64 sums, eps 1e-5) then * weight + bias (libfalcon.cpp:2166-2188)
//   gelu        ggml.c:3477-3484    fp16 table lookup (table built on the host exactly like ggml.c:4276-4290)
//   rope        ggml.c:12957-12978  NeoX pairing (i, i+32); cos/sin come from a host-built table whose theta is
//                                   advanced by repeated f32 multiplication like the reference loop
// (the prompt attention, the block's other non-mat-mul op: kernels_attn.hip)
// Built with -ffp-contract=off.
#include "fq_block_dev.h"
#include "kernels.h"
#include "hip_context.h"
#include <vector>

// ------------------------------------------------------------------------------------------------ layer norm
// one 256-thread workgroup per row; the row lives in LDS between the passes
__global__ void __launch_bounds__(256) k_layer_norm(const float * __restrict__ x, int64_t n, const float * __restrict__ w,
                                                    const float * __restrict__ b, float * __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    float  * row = (float *) smem;
    double * red = (double *)(smem + ((n * 4 + 15) & ~(int64_t) 15));
    layer_norm_row_block(x + (int64_t) blockIdx.x * n, n, w, b, row, red);
    float * yr = y + (int64_t) blockIdx.x * n;
    for (int64_t i = threadIdx.x; i < (n >> 2); i += blockDim.x) ((float4 *) yr)[i] = ((const float4 *) row)[i];
}

// layer norm + the mat-mul's activation quantizer in one launch (prefill): the normalised row goes from LDS straight into
// the Q8 image; y (optional) also receives the f32 row. Same device functions as k_layer_norm + k_quantize_q8*.
template <int ACT>
__global__ void __launch_bounds__(256) k_layer_norm_quant(const float * __restrict__ x, int64_t n, const float * __restrict__ w,
                                                          const float * __restrict__ b, float * __restrict__ y, fq_act a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    float  * row = (float *) smem;
    double * red = (double *)(smem + ((n * 4 + 15) & ~(int64_t) 15));
    layer_norm_row_block(x + (int64_t) blockIdx.x * n, n, w, b, row, red);
    if (y) {
        float * yr = y + (int64_t) blockIdx.x * n;
        for (int64_t i = threadIdx.x; i < (n >> 2); i += blockDim.x) ((float4 *) yr)[i] = ((const float4 *) row)[i];
    }
    __syncthreads();
    uint8_t * col = a.base + (size_t) blockIdx.x * fq_act_col_bytes(ACT, n);
    quantize_row_block<ACT>(row, n, act_image_at(col, ACT, n));
}
// LayerNorm rows live in LDS: n floats + 64 bytes of reduction space. A row must be whole float4 vectors (the kernels move it that way) and fit the CU's 160 KiB; beyond the
// default 64 KiB the kernel is granted its dynamic LDS first, like every launcher here (a runtime may refuse the launch without the grant, and a refused launch
// leaves y stale without a word). false: message, nothing to launch.
static bool layer_norm_row_ok(const char * what, int64_t n, size_t lds) {
    if (n > 0 && n % 4 == 0 && lds <= 160 * 1024) return true;
    fprintf(stderr, "ggml-hip: %s: rows of %lld values unsupported (the row length must be a multiple of 4 and at most %d): nothing launched\n", what, (long long) n, (160 * 1024 - 64) / 4);
    return false;
}
#define FQ_LN_GRANT(KERNEL) { static size_t gmax = 64 * 1024; if (lds > gmax) { HIP_CHECK(hipFuncSetAttribute((const void *) KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds)); gmax = lds; } }
void fq_launch_layer_norm_quant(const float * x, int64_t n, int64_t rows, const float * w, const float * b, float * y, const fq_act & a, hipStream_t st) {
    FQ_TL(st, "layer_norm_quant");
    const size_t lds = ((n * 4 + 15) & ~(size_t) 15) + 64;
    if (!layer_norm_row_ok("layer_norm_quant", n, lds)) return;
#define FQ_LNQ(A) { FQ_LN_GRANT(k_layer_norm_quant<A>) hipLaunchKernelGGL(k_layer_norm_quant<A>, dim3((unsigned) rows), dim3(256), lds, st, x, n, w, b, y, a); }
    if (a.type == FQ_Q8_0) FQ_LNQ(FQ_Q8_0) else if (a.type == FQ_Q8_1) FQ_LNQ(FQ_Q8_1) else FQ_LNQ(FQ_Q8_K)
#undef FQ_LNQ
}

// x = (a + b) + x: the residual sum of a block (libfalcon.cpp:2399-2400: inpL = (ffn_out + attn_out) + inpL) as a launch of its own -- the short prompts' two-stream form,
// where neither mat-mul should wait for the other just to carry the sum in its epilogue (falcon_stage.hip)
__global__ void __launch_bounds__(256) k_add2_inplace(float * __restrict__ x, const float * __restrict__ a, const float * __restrict__ b, int64_t nv) {
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (int64_t) gridDim.x * blockDim.x) {
        const float4 p = ((const float4 *) a)[i], q = ((const float4 *) b)[i]; float4 v = ((float4 *) x)[i];
        v.x = (p.x + q.x) + v.x; v.y = (p.y + q.y) + v.y; v.z = (p.z + q.z) + v.z; v.w = (p.w + q.w) + v.w;
        ((float4 *) x)[i] = v;
    }
}
void fq_launch_add2_inplace(float * x, const float * a, const float * b, int64_t n, hipStream_t st) {
    FQ_TL(st, "add2");
    const int64_t nv = n >> 2;
    const unsigned grid = (unsigned)((nv + 255) / 256 < 2048 ? (nv + 255) / 256 : 2048);
    hipLaunchKernelGGL(k_add2_inplace, dim3(grid ? grid : 1), dim3(256), 0, st, x, a, b, nv);
}

// ... and, one workgroup per token, with the LayerNorm(s) + activation image(s) that follow (fq_next_norm): the sum, then k_layer_norm_quant's own device code on the row it left
// in LDS (per thread the same elements in the same order: the same f64 sums, the same bits); a second norm of a two-norm block repeats only * w + b
template <int ACT>
__global__ void __launch_bounds__(256) k_add2_ln(float * __restrict__ x, const float * __restrict__ a, const float * __restrict__ b, int64_t n, fq_next_norm nn) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const size_t rowb = ((size_t) n * 4 + 15) & ~(size_t) 15;
    float  * row = (float *) smem;
    float  * out = nn.w1 ? (float *)(smem + rowb) : row;
    double * red = (double *)(smem + (nn.w1 ? 2 : 1) * rowb);
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t) blockIdx.x * n, nv = n >> 2;
    double s = 0.0;
    for (int64_t i = tid; i < nv; i += 256) {
        const float4 p = ((const float4 *)(a + r0))[i], q = ((const float4 *)(b + r0))[i]; float4 v = ((float4 *)(x + r0))[i];
        v.x = (p.x + q.x) + v.x; v.y = (p.y + q.y) + v.y; v.z = (p.z + q.z) + v.z; v.w = (p.w + q.w) + v.w;
        ((float4 *)(x + r0))[i] = v; ((float4 *) row)[i] = v;
        s += (double) v.x; s += (double) v.y; s += (double) v.z; s += (double) v.w;
    }
    layer_norm_from_row(s, n, nn.w0, nn.b0, row, out, red);
    quantize_row_block<ACT>(out, n, act_image_at(nn.a0.base + (size_t) blockIdx.x * fq_act_col_bytes(ACT, n), ACT, n));
    if (nn.w1) {
        __syncthreads();
        layer_norm_apply(n, nn.w1, nn.b1, row, out);
        quantize_row_block<ACT>(out, n, act_image_at(nn.a1.base + (size_t) blockIdx.x * fq_act_col_bytes(ACT, n), ACT, n));
    }
}
bool fq_add2_ln_ok(const fq_next_norm & nn, int64_t E) {
    static const bool on = !(getenv("FALCON_HIP_ADD2_LN") && atoi(getenv("FALCON_HIP_ADD2_LN")) == 0);
    if (!on || !nn.w0 || E % 4 || nn.a0.K != E || (nn.w1 && (nn.a1.type != nn.a0.type || nn.a1.K != E))) return false;
    if (nn.a0.type != FQ_Q8_0 && nn.a0.type != FQ_Q8_1 && nn.a0.type != FQ_Q8_K) return false;
    if (nn.a0.type == FQ_Q8_K ? E % 256 : E % 32) return false;
    return (nn.w1 ? 2 : 1) * (((size_t) E * 4 + 15) & ~(size_t) 15) + 64 <= 160 * 1024;
}
void fq_launch_add2_ln(float * x, const float * a, const float * b, int64_t E, int64_t rows, const fq_next_norm & nn, hipStream_t st) {
    FQ_TL(st, "add2_ln");
    const size_t lds = (nn.w1 ? 2 : 1) * (((size_t) E * 4 + 15) & ~(size_t) 15) + 64;
#define FQ_A2LN(A) { static size_t gmax = 64 * 1024; if (lds > gmax) { HIP_CHECK(hipFuncSetAttribute((const void *) k_add2_ln<A>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds)); gmax = lds; } \
        hipLaunchKernelGGL(k_add2_ln<A>, dim3((unsigned) rows), dim3(256), lds, st, x, a, b, E, nn); }
    if (nn.a0.type == FQ_Q8_0) FQ_A2LN(FQ_Q8_0) else if (nn.a0.type == FQ_Q8_1) FQ_A2LN(FQ_Q8_1) else FQ_A2LN(FQ_Q8_K)
#undef FQ_A2LN
}

// two norms of the same rows in one launch (Falcon-40B's ln_mlp and ln_attn: blockIdx.y picks the weights and the image)
template <int ACT>
__global__ void __launch_bounds__(256) k_layer_norm_quant2(const float * __restrict__ x, int64_t n, const float * __restrict__ w0, const float * __restrict__ b0, fq_act a0,
                                                           const float * __restrict__ w1, const float * __restrict__ b1, fq_act a1) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    float  * row = (float *) smem;
    double * red = (double *)(smem + ((n * 4 + 15) & ~(int64_t) 15));
    const bool second = blockIdx.y != 0;
    layer_norm_row_block(x + (int64_t) blockIdx.x * n, n, second ? w1 : w0, second ? b1 : b0, row, red);
    __syncthreads();
    uint8_t * col = (second ? a1.base : a0.base) + (size_t) blockIdx.x * fq_act_col_bytes(ACT, n);
    quantize_row_block<ACT>(row, n, act_image_at(col, ACT, n));
}
bool fq_launch_layer_norm_quant2(const float * x, int64_t n, int64_t rows, const float * w0, const float * b0, const fq_act & a0,
                                 const float * w1, const float * b1, const fq_act & a1, hipStream_t st) {
    FQ_TL(st, "layer_norm_quant2");
    if (a0.type != a1.type) return false;
    const size_t lds = ((n * 4 + 15) & ~(size_t) 15) + 64;
    if (!layer_norm_row_ok("layer_norm_quant2", n, lds)) return false;
    const dim3 grid((unsigned) rows, 2);
#define FQ_LNQ2(A) { FQ_LN_GRANT(k_layer_norm_quant2<A>) hipLaunchKernelGGL(k_layer_norm_quant2<A>, grid, dim3(256), lds, st, x, n, w0, b0, a0, w1, b1, a1); }
    if (a0.type == FQ_Q8_0) FQ_LNQ2(FQ_Q8_0) else if (a0.type == FQ_Q8_1) FQ_LNQ2(FQ_Q8_1) else FQ_LNQ2(FQ_Q8_K)
#undef FQ_LNQ2
    return true;
}

void fq_launch_layer_norm(const float * x, int64_t n, int64_t rows, const float * w, const float * b, float * y, hipStream_t st) {
    FQ_TL(st, "layer_norm");
    const size_t lds = ((n * 4 + 15) & ~(size_t) 15) + 64;
    if (!layer_norm_row_ok("layer_norm", n, lds)) return;
    FQ_LN_GRANT(k_layer_norm)
    hipLaunchKernelGGL(k_layer_norm, dim3((unsigned) rows), dim3(256), lds, st, x, n, w, b, y);
}
#undef FQ_LN_GRANT

// ------------------------------------------------------------------------------------------------ gelu / add
__global__ void k_gelu(const float * __restrict__ x, float * __restrict__ y, int64_t n, const uint16_t * __restrict__ tab) {
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t) gridDim.x * blockDim.x)
        y[i] = h2f_bits(tab[f2h_bits(x[i])]);
}
void fq_launch_gelu(const float * x, float * y, int64_t n, const uint16_t * gelu_table, hipStream_t st) {
    FQ_TL(st, "gelu");
    const int blocks = (int) ((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256);
    hipLaunchKernelGGL(k_gelu, dim3(blocks), dim3(256), 0, st, x, y, n, gelu_table);
}
__global__ void k_add3(const float * __restrict__ a, const float * __restrict__ b, const float * __restrict__ c, float * __restrict__ y, int64_t n) {
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t) gridDim.x * blockDim.x)
        y[i] = (a[i] + b[i]) + c[i];
}
void fq_launch_add3(const float * a, const float * b, const float * c, float * y, int64_t n, hipStream_t st) {
    FQ_TL(st, "add3");
    const int blocks = (int) ((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256);
    hipLaunchKernelGGL(k_add3, dim3(blocks), dim3(256), 0, st, a, b, c, y, n);
}

// ------------------------------------------------------------------------------------------------ rope + KV append
// thread = one rotation pair (or one V element pair). Heads 0..H-1 are Q (rotated in place), H..H+HKV-1 are K
// (rotated into the cache), H+HKV.. are V (copied into the cache). Caches: [n_ctx][HKV][D] f32 for this layer.
// seq_stride > 0: the N rows are N independent sequences at the SAME position n_past, row t owning the cache at
// kc / vc + t * seq_stride (lock-step decode streams of one pipeline stage step); with pos_stride 1 row t sits at its own
// position n_past_ptr[t] instead (ragged steps, falcon_hip_eval_seqs)
__global__ void k_rope_kv(float * __restrict__ qkv, int N, int H, int HKV, int D, const int * __restrict__ n_past_ptr, const float * __restrict__ cs,
                          float * __restrict__ kc, float * __restrict__ vc, int64_t seq_stride, int pos_stride) {
    const int half = D >> 1;
    const int heads = H + 2 * HKV;
    const int n_past = *n_past_ptr;          // device scalar: one captured hipGraph serves every decode step
    const int64_t total = (int64_t) N * heads * half;
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t) gridDim.x * blockDim.x) {
        const int k = (int)(i % half);
        const int h = (int)((i / half) % heads);
        const int t = (int)(i / ((int64_t) half * heads));
        float * v = qkv + ((int64_t) t * heads + h) * D;
        const int pos = seq_stride ? n_past_ptr[(int64_t) t * pos_stride] : n_past + t;
        float * kcs = kc + (int64_t) t * seq_stride, * vcs = vc + (int64_t) t * seq_stride;
        if (h < H + HKV) {
            const float c = cs[((int64_t) pos * half + k) * 2], s = cs[((int64_t) pos * half + k) * 2 + 1];
            const float x0 = v[k], x1 = v[k + half];
            const float r0 = x0 * c - x1 * s, r1 = x0 * s + x1 * c;     // ggml.c:12974-12975
            if (h < H) { v[k] = r0; v[k + half] = r1; }
            else { float * o = kcs + ((int64_t) pos * HKV + (h - H)) * D; o[k] = r0; o[k + half] = r1; }
        } else {
            float * o = vcs + ((int64_t) pos * HKV + (h - H - HKV)) * D;
            o[k] = v[k]; o[k + half] = v[k + half];
        }
    }
}
void fq_launch_rope_kv(float * qkv, int N, int H, int HKV, int D, const int * n_past_dev, const float * rope_cs, float * k_cache, float * v_cache, hipStream_t st,
                       int64_t seq_stride, int pos_stride) {
    FQ_TL(st, "rope_kv");
    const int64_t total = (int64_t) N * (H + 2 * HKV) * (D / 2);
    const int blocks = (int) ((total + 255) / 256 > 8192 ? 8192 : (total + 255) / 256);
    hipLaunchKernelGGL(k_rope_kv, dim3(blocks), dim3(256), 0, st, qkv, N, H, HKV, D, n_past_dev, rope_cs, k_cache, v_cache, seq_stride, seq_stride ? pos_stride : 0);
}

// ------------------------------------------------------------------------------------------------ self-test
// DPP/readlane wave reductions against the plain __shfl_xor butterfly (same pairing order): must agree bit for bit.
__global__ void k_selftest_reduce(int * __restrict__ mismatches, unsigned seed) {
    const int lane = threadIdx.x & 63;
    unsigned h = seed ^ (blockIdx.x * 2654435761u) ^ (threadIdx.x * 40503u);
    for (int it = 0; it < 64; ++it) {
        h = h * 1664525u + 1013904223u;
        const float  f = __builtin_bit_cast(float, (h & 0x007FFFFFu) | 0x3F800000u) * ((h >> 24) & 1 ? -3.7f : 1.3f) * (float)(1 + (h >> 28));
        const double d = (double) f * 1.000000119 + 1e-9 * (double)(h & 1023);
        const int    i = (int)(h >> 7) - (1 << 23);
        const float  fa = wave_reduce(f, op_add()), fb = wave_reduce_shfl(f, op_add());
        const double da = wave_reduce(d, op_add()), db = wave_reduce_shfl(d, op_add());
        const int    ia = wave_reduce(i, op_add()), ib = wave_reduce_shfl(i, op_add());
        const float  ma = wave_reduce(f, op_max()), mb = wave_reduce_shfl(f, op_max());
        int bad = 0;
        bad += __builtin_bit_cast(int, fa) != __builtin_bit_cast(int, fb);
        bad += __builtin_bit_cast(long long, da) != __builtin_bit_cast(long long, db);
        bad += ia != ib;
        bad += __builtin_bit_cast(int, ma) != __builtin_bit_cast(int, mb);
        if (bad) atomicAdd(mismatches, bad);
        (void) lane;
    }
}
int fq_selftest_reduce(hipStream_t st) {
    int * dev = nullptr; int host = -1;
    HIP_CHECK(hipMalloc((void **) &dev, 4));
    HIP_CHECK(hipMemsetAsync(dev, 0, 4, st));
    hipLaunchKernelGGL(k_selftest_reduce, dim3(64), dim3(256), 0, st, dev, 12345u);
    HIP_CHECK(hipMemcpyAsync(&host, dev, 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipFree(dev));
    return host;
}

// ---- exp_f16_formula (fq_device.h) against the host-built table, every non-NaN fp16 input
__global__ void k_verify_exp_formula(const uint16_t * __restrict__ table, int * mismatches) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 65536u) return;
    if ((i & 0x7C00u) == 0x7C00u && (i & 0x03FFu)) return;      // NaN in: NaN out either way, payloads are not compared
    if (exp_f16_formula((uint16_t) i) != table[i]) atomicAdd(mismatches, 1);
}
// diagnostic: the inputs exp_f16_fast leaves undecided, with the table's entries: (bits << 16 | entry), ascending; returns their number
__global__ void k_exp_boundary(const uint16_t * __restrict__ table, unsigned * __restrict__ flags) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 65536u) return;
    uint16_t h;
    const bool nan = (i & 0x7C00u) == 0x7C00u && (i & 0x03FFu);
    flags[i] = (!nan && !exp_f16_fast((uint16_t) i, h)) ? ((i << 16) | table[i]) : 0xFFFFFFFFu;
}
int fq_exp_boundary(const uint16_t * exp_table, unsigned * out_host, int cap, hipStream_t st) {
    unsigned * d = nullptr;
    HIP_CHECK(hipMalloc((void **) &d, 65536 * 4));
    hipLaunchKernelGGL(k_exp_boundary, dim3(256), dim3(256), 0, st, exp_table, d);
    std::vector<unsigned> f(65536);
    HIP_CHECK(hipMemcpyAsync(f.data(), d, 65536 * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipFree(d));
    int n = 0;
    for (unsigned v : f) if (v != 0xFFFFFFFFu) { if (n < cap) out_host[n] = v; ++n; }
    return n;
}
int fq_verify_exp_formula(const uint16_t * exp_table, hipStream_t st) {
    int * d = nullptr; int h = -1;
    HIP_CHECK(hipMalloc((void **) &d, 4));
    HIP_CHECK(hipMemsetAsync(d, 0, 4, st));
    hipLaunchKernelGGL(k_verify_exp_formula, dim3(256), dim3(256), 0, st, exp_table, d);
    HIP_CHECK(hipMemcpyAsync(&h, d, 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipFree(d));
    return h;
}
