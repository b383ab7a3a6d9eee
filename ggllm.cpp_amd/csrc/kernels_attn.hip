// kernels_attn.hip -- the prompt (prefill) attention of a Falcon decoder block, device resident (gfx950): its kernels, fq_launch_attention, and the draft-and-verify
// pair. In the reference this always runs on the CPU (see kernels_block.hip); the arithmetic follows the CPU ops:
//   attention   K.Q (ggml.c:11049-11088, GQA broadcast i02 = i12/(H/HKV)), scale, causal mask (ggml.c:12300-12351),
//               soft_max with the fp16 exp table and an f64 sum (ggml.c:12389-12456), V.P
// WHICH kernel a launch takes, with what grid, LDS and scratch, is decided in fq_attn_forms.h (fq_attn_plan_of), where every FQ_ATTN_* switch is named;
// fq_launch_attention below only launches the plan.
// Built with -ffp-contract=off.
#include "fq_block_dev.h"
#include "fq_attn_dev.h"
#include "fq_attn_forms.h"
#include "kernels.h"
#include "hip_context.h"

// grant a kernel its dynamic LDS beyond the default 64 KiB, once per size reached (a runtime may refuse the launch without the grant)
template <auto KERNEL>
static void attn_grant_lds(size_t lds) {
    static size_t granted = 64 * 1024;
    if (lds > granted) { HIP_CHECK(hipFuncSetAttribute((const void *) KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds)); granted = lds; }
}

// ------------------------------------------------------------------------------------------------ attention
// One 256-thread workgroup per (head, token); n_kv = n_past + t + 1 keys are visible, all read from the KV cache
// (k_rope_kv has already appended this launch's keys). The arithmetic lives in fq_attn_dev.h.
template <bool F64>
__global__ void __launch_bounds__(256) k_attention(const float * __restrict__ qkv, int H, int HKV, const int * __restrict__ n_past_ptr,
                                                   const float * __restrict__ kc, const float * __restrict__ vc,
                                                   const uint16_t * __restrict__ exp_tab, float * __restrict__ att, int64_t seq_stride, int pos_stride) {
    constexpr int D = 64;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int h = blockIdx.x, t = blockIdx.y;
    const int n_kv = (seq_stride ? n_past_ptr[(int64_t) t * pos_stride] : *n_past_ptr + t) + 1;      // (pos_stride 1: row t at its own position)
    kc += (int64_t) t * seq_stride; vc += (int64_t) t * seq_stride;
    const int heads = H + 2 * HKV;
    const int hk = h / (H / HKV);
    const attn_lds L = attn_lds_carve(smem);
    const float o = attn_head_block<F64>(qkv + ((int64_t) t * heads + h) * D, kc, vc, HKV, hk, n_kv, nullptr, nullptr, exp_tab, L);
    if (threadIdx.x < 64) att[(int64_t) t * H * D + (int64_t) h * D + threadIdx.x] = o;
}

// R consecutive tokens of a head per workgroup (prefill): key / value tiles are loaded once per R tokens (fq_attn_dev.h)
template <int R, bool F64>
__global__ void __launch_bounds__(256) k_attention_rows(const float * __restrict__ qkv, int N, int H, int HKV, const int * __restrict__ n_past_ptr,
                                                        const float * __restrict__ kc, const float * __restrict__ vc,
                                                        const uint16_t * __restrict__ exp_tab, float * __restrict__ att, int p_stride,
                                                        float * __restrict__ p_scratch) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int h = blockIdx.x, t0 = blockIdx.y * R;
    const int nrows = N - t0 < R ? N - t0 : R;
    float * redf = (float *) smem;
    double * red = (double *)(smem + 64);
    // the R score rows: LDS, or (long contexts) this workgroup's own slice of a global scratch buffer -- written and read
    // back by the same workgroup within microseconds (L2 / Infinity Cache), and the LDS they would take no longer limits
    // the number of workgroups per CU
    float * p = p_scratch ? p_scratch + ((size_t) blockIdx.y * gridDim.x + blockIdx.x) * (size_t) R * (size_t) p_stride
                          : (float *)(smem + 64 + 16 * 64 * 8);
    attn_rows_block<R, F64>(qkv, H + 2 * HKV, h, t0, nrows, *n_past_ptr, kc, vc, HKV, h / (H / HKV), exp_tab, redf, red, p, p_stride, att, H);
}
// ---- prefill attention on the f32 matrix pipe (N >= 32) ----------------------------------------------------------------------
// v_mfma_f32_32x32x2_f32 performs, per output element, ONE fused multiply-add per k step in ascending k
// (scripts/microbench/mb_mfma_f32.hip: 0 of 1024 outputs differ from the fmaf chain over 64 steps) -- the arithmetic of the
// reference's SIMD builds (f32 FMA accumulation, ggml.c:2270-2294) with a SEQUENTIAL association the oracle restates in two
// lines (oracle_falcon.c dot_qk_mfma / dot_pv_mfma):
//   score(i, j) = chain over s = 0..31 of  q[s] k[s],  q[32 + s] k[32 + s]            (lanes 0-31 feed dims 0..31, lanes 32-63 dims 32..63)
//   out(i, d)   = E + O,  E / O = chains over the even / odd 32-key tiles, in a tile over s = 0..15 of  p[s] v[s],  p[16 + s] v[16 + s]
// One workgroup = one head x 32 query tokens, 4 waves: the waves split the key tiles of K.Q (one 32 x 32 score tile = 32
// MFMAs), the soft_max rows (max, fp16-table exp, f64 sum -- exact in any order: <= 2^13 fp16-valued terms --, scaling), and
// V.P as (dim half) x (tile parity). Scores / probabilities live in the workgroup's slice of the global scratch (L2).
typedef float v16f __attribute__((ext_vector_type(16)));
__global__ void __launch_bounds__(256) k_attention_mfma(const float * __restrict__ qkv, int N, int H, int HKV, const int * __restrict__ n_past_ptr,
                                                        const float * __restrict__ kc, const float * __restrict__ vc,
                                                        const uint16_t * __restrict__ exp_tab, float * __restrict__ att, int p_stride,
                                                        float * __restrict__ p_scratch) {
    __shared__ float xch[2][16][64];
    __shared__ float rmax[4][32], rinv[32];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, li = lane & 31, hf = lane >> 5;
    const int h = blockIdx.x, i0 = blockIdx.y * 32, hk = h / (H / HKV), heads = H + 2 * HKV;
    const int n_past = *n_past_ptr;
    const int nrows = N - i0 < 32 ? N - i0 : 32;
    const int n_kv_max = n_past + i0 + nrows;                       // keys the tile's last token sees
    const int n_rows_cache = n_past + N;                            // key / value rows that exist
    const int ntile = (n_kv_max + 31) >> 5;
    float * p = p_scratch + ((size_t) blockIdx.y * gridDim.x + blockIdx.x) * (size_t) 32 * (size_t) p_stride;
    // The score matrix makes FOUR trips through the scratch (written here, read + rewritten as exp() by the soft_max, read by V.P):
    // the row maxima are taken from the MFMA results in registers, and the 1 / sum scaling is applied to the operand V.P loads
    // (p = e * inv, the soft_max's own rounding) -- the scratch of a 2048-token prompt is 1.2 GB and does not stay in the caches.
    // ---- scores
    {
        f32x4 q8[8];
        const float * qrow = qkv + ((int64_t)(i0 + (li < nrows ? li : nrows - 1)) * heads + h) * 64 + 32 * hf;
#pragma unroll
        for (int v = 0; v < 8; ++v) q8[v] = ((const f32x4 *) qrow)[v];
        auto load_k = [&](int T, f32x4 (&k8)[8]) {
            const int j = 32 * T + li;
            const float * krow = kc + ((int64_t)(j < n_rows_cache ? j : n_rows_cache - 1) * HKV + hk) * 64 + 32 * hf;
#pragma unroll
            for (int v = 0; v < 8; ++v) k8[v] = ((const f32x4 *) krow)[v];
        };
        f32x4 ka[8], kb[8];
        float mx[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) mx[r] = -INFINITY;
        if (wid < ntile) load_k(wid, ka);
        for (int T = wid; T < ntile; T += 4) {
            if (T + 4 < ntile) load_k(T + 4, kb);
            v16f c = {0};
#pragma unroll
            for (int v = 0; v < 8; ++v) {
                c = __builtin_amdgcn_mfma_f32_32x32x2f32(q8[v].x, ka[v].x, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x2f32(q8[v].y, ka[v].y, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x2f32(q8[v].z, ka[v].z, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x2f32(q8[v].w, ka[v].w, c, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ir = (r & 3) + 8 * (r >> 2) + 4 * hf;
                const float sc = c[r] * 0.125f;
                p[(size_t) ir * p_stride + 32 * T + li] = sc;
                mx[r] = fq_max_f32(mx[r], (ir < nrows && 32 * T + li <= n_past + i0 + ir) ? sc : -INFINITY);
            }
#pragma unroll
            for (int v = 0; v < 8; ++v) ka[v] = kb[v];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float m = reduce32(mx[r], op_max());
            if (li == 0) rmax[wid][(r & 3) + 8 * (r >> 2) + 4 * hf] = m;
        }
    }
    __syncthreads();
    // ---- soft_max: wave w takes rows w, w + 4, ...: exp() of the visible keys, zeros up to the last tile, 1 / sum kept aside
    for (int ir = wid; ir < 32; ir += 4) {
        float * pr = p + (size_t) ir * p_stride;
        const int n_kv = ir < nrows ? n_past + i0 + ir + 1 : 0;
        const float m = fq_max_f32(fq_max_f32(rmax[0][ir], rmax[1][ir]), fq_max_f32(rmax[2][ir], rmax[3][ir]));
        double lsum = 0.0;
#pragma unroll 4
        for (int j = 4 * lane; j < 32 * ntile; j += 256) {
            const f32x4 x = *(const f32x4 *)(pr + j);
            f32x4 e;
            e.x = j     < n_kv ? soft_max_exp(exp_tab, x.x - m) : 0.0f;
            e.y = j + 1 < n_kv ? soft_max_exp(exp_tab, x.y - m) : 0.0f;
            e.z = j + 2 < n_kv ? soft_max_exp(exp_tab, x.z - m) : 0.0f;
            e.w = j + 3 < n_kv ? soft_max_exp(exp_tab, x.w - m) : 0.0f;
            *(f32x4 *)(pr + j) = e;
            lsum += (double) e.x; lsum += (double) e.y; lsum += (double) e.z; lsum += (double) e.w;     // (exact in any order)
        }
        lsum = wave_sum(lsum);
        if (lane == 0) rinv[ir] = (float)(1.0 / lsum);
    }
    __syncthreads();
    // ---- V.P: wave = (dim half, tile parity)
    {
        const int dh = wid & 1, par = wid >> 1;
        const float * prow = p + (size_t) li * p_stride + 16 * hf;
        const float inv = rinv[li];
        auto load_pv = [&](int T, f32x4 (&p4)[4], float (&v16)[16]) {
#pragma unroll
            for (int v = 0; v < 4; ++v) p4[v] = ((const f32x4 *)(prow + 32 * T))[v];
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const int j = 32 * T + 16 * hf + s;
                v16[s] = vc[((int64_t)(j < n_rows_cache ? j : n_rows_cache - 1) * HKV + hk) * 64 + 32 * dh + li];
            }
        };
        f32x4 pa[4], pb[4]; float va[16], vb[16];
        if (par < ntile) load_pv(par, pa, va);
        v16f c = {0};
        for (int T = par; T < ntile; T += 2) {
            if (T + 2 < ntile) load_pv(T + 2, pb, vb);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                c = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[v].x * inv, va[4 * v + 0], c, 0, 0, 0);      // p = e * inv, the rounding of the soft_max's own scaling step (ggml_vec_scale_f32)
                c = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[v].y * inv, va[4 * v + 1], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[v].z * inv, va[4 * v + 2], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[v].w * inv, va[4 * v + 3], c, 0, 0, 0);
            }
#pragma unroll
            for (int v = 0; v < 4; ++v) pa[v] = pb[v];
#pragma unroll
            for (int s = 0; s < 16; ++s) va[s] = vb[s];
        }
        if (par == 1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) xch[dh][r][lane] = c[r];
        }
        __syncthreads();
        if (par == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ir = (r & 3) + 8 * (r >> 2) + 4 * hf;
                if (ir < nrows) att[(int64_t)(i0 + ir) * H * 64 + (int64_t) h * 64 + 32 * dh + li] = c[r] + xch[dh][r][lane];
            }
        }
    }
}

// ---- the same arithmetic with the score rows in LDS: one head x 16 query tokens per workgroup, v_mfma_f32_16x16x4_f32 ------------
// v_mfma_f32_16x16x4_f32 is the same fused chain, four k steps per instruction in ascending k (scripts/microbench/mb_mfma_f32_16.hip:
// 0 of 2048 outputs differ), so the chains above are kept term for term by feeding k = 0..3 of instruction m with
//   K.Q : dims  2m, 32 + 2m, 2m + 1, 33 + 2m     (m = 0..15)        V.P : keys  2m, 16 + 2m, 2m + 1, 17 + 2m  of a 32-key tile (m = 0..7)
// i.e. lane group kq = lane >> 4 holds the even (kq < 2) or odd elements of the low (kq even) or high (kq odd) half. Results are
// bit-identical to k_attention_mfma (and to the oracle's dot_qk_mfma / dot_pv_mfma). 16 rows x n_kv floats fit the LDS up to ~2400
// keys (128 KiB at 2048): the score matrix never leaves the CU -- the 32-row form moves 2.5 GB of HBM traffic per 2048-token
// launch for it. 8 waves: K.Q by 16-key sub-tiles, soft_max two rows per wave, V.P as (16-dim tile) x (32-key tile parity).
typedef float v4f_ __attribute__((ext_vector_type(4)));
__global__ void __launch_bounds__(512) k_attention_mfma16(const float * __restrict__ qkv, int N, int H, int HKV, const int * __restrict__ n_past_ptr,
                                                          const float * __restrict__ kc, const float * __restrict__ vc,
                                                          const uint16_t * __restrict__ exp_tab, float * __restrict__ att, int ps) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    float * p = (float *) smem;                                     // [16][ps], ps = 32 ntile_max + 4
    float * rmax = p + 16 * ps;                                     // [8 waves][16 rows]
    float * rinv = rmax + 8 * 16;                                   // [16]
    float * xch  = rinv + 16;                                       // [4 dim tiles][4][64]
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l16 = lane & 15, kq = lane >> 4;
    const int h = blockIdx.x, i0 = blockIdx.y * 16, hk = h / (H / HKV), heads = H + 2 * HKV;
    const int n_past = *n_past_ptr;
    const int nrows = N - i0 < 16 ? N - i0 : 16;
    const int n_kv_max = n_past + i0 + nrows;                       // keys the tile's last token sees
    const int n_rows_cache = n_past + N;                            // key / value rows that exist
    const int ntile = (n_kv_max + 31) >> 5, nsub = 2 * ntile;
    const int eo = kq >> 1, hi = kq & 1;                            // the lane group's elements: odd (1) / even (0) ones of the high (1) / low (0) half
    // ---- scores
    {
        float q16[16];
        {
            const float * qrow = qkv + ((int64_t)(i0 + (l16 < nrows ? l16 : nrows - 1)) * heads + h) * 64 + 32 * hi;
#pragma unroll
            for (int v = 0; v < 8; ++v) { const f32x4 t = ((const f32x4 *) qrow)[v]; q16[2 * v] = eo ? t.y : t.x; q16[2 * v + 1] = eo ? t.w : t.z; }
        }
        auto load_k = [&](int U, float (&k16)[16]) {
            const int j = 16 * U + l16;
            const float * krow = kc + ((int64_t)(j < n_rows_cache ? j : n_rows_cache - 1) * HKV + hk) * 64 + 32 * hi;
#pragma unroll
            for (int v = 0; v < 8; ++v) { const f32x4 t = ((const f32x4 *) krow)[v]; k16[2 * v] = eo ? t.y : t.x; k16[2 * v + 1] = eo ? t.w : t.z; }
        };
        float ka[16], kb[16];
        float mx[4] = { -INFINITY, -INFINITY, -INFINITY, -INFINITY };
        if (wid < nsub) load_k(wid, ka);
        for (int U = wid; U < nsub; U += 8) {
            if (U + 8 < nsub) load_k(U + 8, kb);
            v4f_ c = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int m = 0; m < 16; ++m) c = __builtin_amdgcn_mfma_f32_16x16x4f32(q16[m], ka[m], c, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ir = 4 * kq + r, j = 16 * U + l16;
                const float sc = c[r] * 0.125f;
                p[ir * ps + j] = sc;
                mx[r] = fq_max_f32(mx[r], (ir < nrows && j <= n_past + i0 + ir) ? sc : -INFINITY);
            }
#pragma unroll
            for (int v = 0; v < 16; ++v) ka[v] = kb[v];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float m = reduce16(mx[r], op_max());
            if (l16 == 0) rmax[wid * 16 + 4 * kq + r] = m;
        }
    }
    __syncthreads();
    // ---- soft_max: wave w takes rows w and w + 8: exp() of the visible keys, zeros up to the last tile, 1 / sum kept aside
    for (int ir = wid; ir < 16; ir += 8) {
        float * pr = p + ir * ps;
        const int n_kv = ir < nrows ? n_past + i0 + ir + 1 : 0;
        float m = rmax[ir];
#pragma unroll
        for (int w2 = 1; w2 < 8; ++w2) m = fq_max_f32(m, rmax[w2 * 16 + ir]);
        double lsum = 0.0;
        for (int j = 4 * lane; j < 32 * ntile; j += 256) {
            const f32x4 x = *(const f32x4 *)(pr + j);
            f32x4 e;
            e.x = j     < n_kv ? soft_max_exp(exp_tab, x.x - m) : 0.0f;
            e.y = j + 1 < n_kv ? soft_max_exp(exp_tab, x.y - m) : 0.0f;
            e.z = j + 2 < n_kv ? soft_max_exp(exp_tab, x.z - m) : 0.0f;
            e.w = j + 3 < n_kv ? soft_max_exp(exp_tab, x.w - m) : 0.0f;
            *(f32x4 *)(pr + j) = e;
            lsum += (double) e.x; lsum += (double) e.y; lsum += (double) e.z; lsum += (double) e.w;     // (exact in any order)
        }
        lsum = wave_sum(lsum);
        if (lane == 0) rinv[ir] = (float)(1.0 / lsum);
    }
    __syncthreads();
    // ---- V.P: wave = (16-dim tile dt, tile parity par)
    {
        const int dt = wid & 3, par = wid >> 2;
        const float * prow = p + l16 * ps + 16 * hi;                // keys 16 hi .. 16 hi + 15 of a tile: the even or the odd ones
        const float inv = rinv[l16];
        auto load_pv = [&](int T, float (&p8)[8], float (&v8)[8]) {
#pragma unroll
            for (int v = 0; v < 4; ++v) { const f32x4 t = ((const f32x4 *)(prow + 32 * T))[v]; p8[2 * v] = eo ? t.y : t.x; p8[2 * v + 1] = eo ? t.w : t.z; }
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const int j = 32 * T + 16 * hi + 2 * m + eo;
                v8[m] = vc[((int64_t)(j < n_rows_cache ? j : n_rows_cache - 1) * HKV + hk) * 64 + 16 * dt + l16];
            }
        };
        float pa[8], pb[8], va[8], vb[8];
        if (par < ntile) load_pv(par, pa, va);
        v4f_ c = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int T = par; T < ntile; T += 2) {
            if (T + 2 < ntile) load_pv(T + 2, pb, vb);
#pragma unroll
            for (int m = 0; m < 8; ++m) c = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[m] * inv, va[m], c, 0, 0, 0);      // p = e * inv, the rounding of the soft_max's own scaling step (ggml_vec_scale_f32)
#pragma unroll
            for (int m = 0; m < 8; ++m) { pa[m] = pb[m]; va[m] = vb[m]; }
        }
        if (par == 1) {
#pragma unroll
            for (int r = 0; r < 4; ++r) xch[(dt * 4 + r) * 64 + lane] = c[r];
        }
        __syncthreads();
        if (par == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ir = 4 * kq + r;
                if (ir < nrows) att[(int64_t)(i0 + ir) * H * 64 + (int64_t) h * 64 + 16 * dt + l16] = c[r] + xch[(dt * 4 + r) * 64 + lane];
            }
        }
    }
}

// ---- the 16-row form with TWO workgroups per CU: the probabilities in LDS as the fp16 values they are -------------------------------
// exp() of the soft_max comes out of a table of fp16 values (ggml.c:10911-10960: table_exp_f16), so an (unscaled) probability is
// stored exactly in 2 bytes: 16 rows x 2048 keys = 64 KiB and two 8-wave workgroups share a CU (k_attention_mfma16 keeps f32 scores:
// 128 KiB, one workgroup). The price: a score must be known in f32 until its row's maximum is, so K.Q runs twice -- pass A keeps only
// the row maxima, pass B repeats the same MFMA chains (same operands, same order: same bits) and stores table[f16(s - max)]; the
// f64 sum of those values is exact in any order (<= 2^13 fp16-valued terms), V.P reads p = (float) e16 * inv as before. Results
// bit-identical to k_attention_mfma / k_attention_mfma16 and to the oracle's dot_qk_mfma / dot_pv_mfma. Measured (Falcon-7B block, 71 heads, one launch;
// profiles/r04_attn_forms.txt): 2048 tokens 1.364 ms against 0.978 (k_attention_mfma) and 1.292 (k_attention_mfma16); 512 tokens 0.137 / 0.114 / 0.103 --
// two workgroups per CU do not pay for the second K.Q: a 16-token tile fetches every key / value row twice as often per query as a 32-token one, and that
// traffic (L2), not the score matrix's trips through HBM, is what the 16-row forms wait for. Opt-in (form 17: fq_attn_forms.h, ggml_hip_debug_attention_form(17)),
// kept with its test. ps: uint16 elements per row (32 ntile_max + 8).
__global__ void __launch_bounds__(512, 4) k_attention_mfma16h(const float * __restrict__ qkv, int N, int H, int HKV, const int * __restrict__ n_past_ptr,
                                                              const float * __restrict__ kc, const float * __restrict__ vc,
                                                              const uint16_t * __restrict__ exp_tab, float * __restrict__ att, int ps) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    float  * rmax = (float *) smem;                                 // [8 waves][16 rows]
    double * rsum = (double *)(rmax + 8 * 16);                      // [8 waves][16 rows]
    float  * xch  = (float *)(rsum + 8 * 16);                       // [4 dim tiles][4][64]
    uint16_t * p  = (uint16_t *)(xch + 4 * 4 * 64);                 // [16][ps]
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l16 = lane & 15, kq = lane >> 4;
    const int h = blockIdx.x, i0 = blockIdx.y * 16, hk = h / (H / HKV), heads = H + 2 * HKV;
    const int n_past = *n_past_ptr;
    const int nrows = N - i0 < 16 ? N - i0 : 16;
    const int n_kv_max = n_past + i0 + nrows;                       // keys the tile's last token sees
    const int n_rows_cache = n_past + N;                            // key / value rows that exist
    const int ntile = (n_kv_max + 31) >> 5, nsub = 2 * ntile;
    const int eo = kq >> 1, hi = kq & 1;                            // the lane group's elements: odd (1) / even (0) ones of the high (1) / low (0) half
    // ---- scores, twice
    {
        float q16[16];
        {
            const float * qrow = qkv + ((int64_t)(i0 + (l16 < nrows ? l16 : nrows - 1)) * heads + h) * 64 + 32 * hi;
#pragma unroll
            for (int v = 0; v < 8; ++v) { const f32x4 t = ((const f32x4 *) qrow)[v]; q16[2 * v] = eo ? t.y : t.x; q16[2 * v + 1] = eo ? t.w : t.z; }
        }
        auto load_k = [&](int U, float (&k16)[16]) {
            const int j = 16 * U + l16;
            const float * krow = kc + ((int64_t)(j < n_rows_cache ? j : n_rows_cache - 1) * HKV + hk) * 64 + 32 * hi;
#pragma unroll
            for (int v = 0; v < 8; ++v) { const f32x4 t = ((const f32x4 *) krow)[v]; k16[2 * v] = eo ? t.y : t.x; k16[2 * v + 1] = eo ? t.w : t.z; }
        };
        float ka[16], kb[16];
        float mx[4] = { -INFINITY, -INFINITY, -INFINITY, -INFINITY };
        // pass A: the row maxima
        if (wid < nsub) load_k(wid, ka);
        for (int U = wid; U < nsub; U += 8) {
            if (U + 8 < nsub) load_k(U + 8, kb);
            v4f_ c = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int m = 0; m < 16; ++m) c = __builtin_amdgcn_mfma_f32_16x16x4f32(q16[m], ka[m], c, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ir = 4 * kq + r, j = 16 * U + l16;
                mx[r] = fq_max_f32(mx[r], (ir < nrows && j <= n_past + i0 + ir) ? c[r] * 0.125f : -INFINITY);
            }
#pragma unroll
            for (int v = 0; v < 16; ++v) ka[v] = kb[v];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float m = reduce16(mx[r], op_max());
            if (l16 == 0) rmax[wid * 16 + 4 * kq + r] = m;
        }
        if (wid < nsub) load_k(wid, ka);                            // (pass B's first keys: requested before the barrier)
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float m = rmax[4 * kq + r];
#pragma unroll
            for (int w2 = 1; w2 < 8; ++w2) m = fq_max_f32(m, rmax[w2 * 16 + 4 * kq + r]);
            mx[r] = m;
        }
        // pass B: the same chains again; exp() of the visible keys as fp16 bits, zeros up to the last tile, the sums aside
        double ls[4] = { 0.0, 0.0, 0.0, 0.0 };
        for (int U = wid; U < nsub; U += 8) {
            if (U + 8 < nsub) load_k(U + 8, kb);
            v4f_ c = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int m = 0; m < 16; ++m) c = __builtin_amdgcn_mfma_f32_16x16x4f32(q16[m], ka[m], c, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ir = 4 * kq + r, j = 16 * U + l16;
                uint16_t e = 0;
                if (ir < nrows && j <= n_past + i0 + ir) { const uint16_t hb = f2h_bits(c[r] * 0.125f - mx[r]); e = exp_tab ? exp_tab[hb] : exp_f16_formula(hb); }
                p[ir * ps + j] = e;
                ls[r] += (double) h2f_bits(e);                                                           // (exact in any order)
            }
#pragma unroll
            for (int v = 0; v < 16; ++v) ka[v] = kb[v];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double t = ls[r];
            t += __shfl_xor(t, 1); t += __shfl_xor(t, 2); t += __shfl_xor(t, 4); t += __shfl_xor(t, 8);
            if (l16 == 0) rsum[wid * 16 + 4 * kq + r] = t;
        }
    }
    __syncthreads();
    // ---- V.P: wave = (16-dim tile dt, tile parity par)
    {
        const int dt = wid & 3, par = wid >> 2;
        const uint16_t * prow = p + l16 * ps + 16 * hi;             // keys 16 hi .. 16 hi + 15 of a tile: the even or the odd ones
        double sum = rsum[l16];
#pragma unroll
        for (int w2 = 1; w2 < 8; ++w2) sum += rsum[w2 * 16 + l16];
        const float inv = (float)(1.0 / sum);
        auto load_pv = [&](int T, fq_u4 (&p2)[2], float (&v8)[8]) {
            p2[0] = *(const fq_u4 *)(prow + 32 * T); p2[1] = *(const fq_u4 *)(prow + 32 * T + 8);
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const int j = 32 * T + 16 * hi + 2 * m + eo;
                v8[m] = vc[((int64_t)(j < n_rows_cache ? j : n_rows_cache - 1) * HKV + hk) * 64 + 16 * dt + l16];
            }
        };
        // element 2 m + eo of the 16 halves: the low (eo = 0) or high half of word m
        auto pe = [&](const fq_u4 (&p2)[2], int m) {
            const fq_u4 & q = p2[m >> 2];
            const uint32_t w = (m & 3) == 0 ? q.x : ((m & 3) == 1 ? q.y : ((m & 3) == 2 ? q.z : q.w));
            return h2f_bits((uint16_t)(eo ? w >> 16 : w & 0xFFFFu));
        };
        fq_u4 pa[2], pb[2]; float va[8], vb[8];
        if (par < ntile) load_pv(par, pa, va);
        v4f_ c = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int T = par; T < ntile; T += 2) {
            if (T + 2 < ntile) load_pv(T + 2, pb, vb);
#pragma unroll
            for (int m = 0; m < 8; ++m) c = __builtin_amdgcn_mfma_f32_16x16x4f32(pe(pa, m) * inv, va[m], c, 0, 0, 0);      // p = e * inv, the rounding of the soft_max's own scaling step (ggml_vec_scale_f32)
            pa[0] = pb[0]; pa[1] = pb[1];
#pragma unroll
            for (int m = 0; m < 8; ++m) va[m] = vb[m];
        }
        if (par == 1) {
#pragma unroll
            for (int r = 0; r < 4; ++r) xch[(dt * 4 + r) * 64 + lane] = c[r];
        }
        __syncthreads();
        if (par == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ir = 4 * kq + r;
                if (ir < nrows) att[(int64_t)(i0 + ir) * H * 64 + (int64_t) h * 64 + 16 * dt + l16] = c[r] + xch[(dt * 4 + r) * 64 + lane];
            }
        }
    }
}

// 1: the two dot products of the attention accumulate f32 products in f64 like the reference's portable build (fq_attn_dev.h)

// ---- prefill attention with the probabilities resident in LDS, 32 query tokens per workgroup ("flash" form, round 5: the default while the rows fit) -------
// The arithmetic of k_attention_mfma, operand for operand (v_mfma_f32_32x32x2_f32 chains: score(i, j) over s = 0..31 of dims s, 32 + s; out = E + O, the chains
// over the even / odd 32-key tiles, in a tile over s = 0..15 of keys s, 16 + s; soft_max: max, table[f16(s - max)], exact f64 sum, p = e * (float)(1 / sum)) --
// bit-identical to it and to the oracle's dot_qk_mfma / dot_pv_mfma -- but no score ever leaves the CU: the scratch form moves the N x n_kv score matrix through
// HBM four times (1.25 GB per Falcon-7B launch at 2048 tokens, 17 x the q / K / V / output bytes). A score must be known in f32 until its row's maximum is, and
// exp() comes out of a table of fp16 values (ggml.c:10911-10960), so:
//   pass A   K.Q on the matrix pipe; a wave keeps the f32 scores of ITS tiles in registers (KEEP, <= 2048 keys: 8 tiles x 16 registers; beyond that only the row
//            maxima are kept and pass B runs the same chains again -- same operands, same order: the same bits); row maxima through 1 KiB of LDS
//   pass B   e = table[f16(s - max)] stored as the 2-byte value it is: 32 rows x n_kv x 2 B of LDS (128 KiB at 2048 keys); row sums as exact integers, f64 across waves
//   pass C   V.P with p = (float) e16 * inv, formed one tile ahead of the matrix instructions that take it
// 8 waves: passes A and B deal the 32-key tiles round-robin (two waves per SIMD; key tiles go from L2 straight to registers one tile ahead, a tile is used by one
// wave only); pass C is four chains (dim half x tile parity: the association fixes that) on waves 0-3, one per SIMD, value tiles three ahead. Workgroups are
// PERSISTENT from 4 items per CU on (one per CU, items = (head, query tile) handed out by a counter, heavy query tiles first). Two units of f32 matrix work at the
// pipe's measured rate (one v_mfma_f32_32x32x2_f32 per 30.5 ns and SIMD, and vector instructions do NOT overlap it: scripts/microbench/mb_mfma_f32_*.hip): 0.28 ms
// per Falcon-7B block at 2048 tokens; measured 0.75 (NOTEBOOK 9.1: value loads and p-forming in front of pass C's one wave per SIMD, item turnover).
// pitch_h: halfwords per LDS row = 32 ntile_max + 8 (row pitch 16 bytes off a multiple of 64: conflict-free b128 reads down a column of rows).
// Loads: compiler-managed (FQ_FLASH_PLAIN). The first versions requested the tiles by inline assembly with hand-counted waits tied to the destination registers ("+v")
// because hipcc sinks a plain prefetch load down to its first use -- measured: the same speed (the passes are not bound by load latency), so the plain form is the default.
#ifndef FQ_FLASH_PLAIN
#define FQ_FLASH_PLAIN 1            // 1 (default): compiler-managed loads. 0: the tiles requested by inline-asm loads one / two tiles ahead with hand-counted waits -- measured the SAME speed on MI355X (0.926 against 0.922 ms per 2048-token Falcon-7B launch: the passes are not bound by load latency) and, on one box of the pool, intermittently wrong in tiles whose waves do not all hold keys (scripts/gpu_attn_bisect.py): off
#endif
#if FQ_FLASH_PLAIN
template <int OFF> __device__ __forceinline__ void fl_gload4(f32x4 & d, const float * p) { d = *(const f32x4 *)((const char *) p + OFF); }
__device__ __forceinline__ void fl_gload1(float & d, const float * p) { d = *p; }
#define FL_WAIT8(n, a)  do { } while (0)
#define FL_WAIT16(n, a) do { } while (0)
#else
template <int OFF> __device__ __forceinline__ void fl_gload4(f32x4 & d, const float * p) { asm volatile("global_load_dwordx4 %0, %1, off offset:%2" : "=v"(d) : "v"(p), "n"(OFF)); }
__device__ __forceinline__ void fl_gload1(float & d, const float * p) { asm volatile("global_load_dword %0, %1, off" : "=v"(d) : "v"(p)); }
#define FL_WAIT8(n, a)  asm volatile("s_waitcnt vmcnt(" #n ")" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]))
#define FL_WAIT16(n, a) asm volatile("s_waitcnt vmcnt(" #n ")" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]), \
                                                                "+v"(a[8]), "+v"(a[9]), "+v"(a[10]), "+v"(a[11]), "+v"(a[12]), "+v"(a[13]), "+v"(a[14]), "+v"(a[15]))
#endif
#define FL_QK(c, k8) _Pragma("unroll") for (int v_ = 0; v_ < 8; ++v_) { \
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(q8[v_].x, k8[v_].x, c, 0, 0, 0); c = __builtin_amdgcn_mfma_f32_32x32x2f32(q8[v_].y, k8[v_].y, c, 0, 0, 0); \
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(q8[v_].z, k8[v_].z, c, 0, 0, 0); c = __builtin_amdgcn_mfma_f32_32x32x2f32(q8[v_].w, k8[v_].w, c, 0, 0, 0); }
// k_attn_pack_k: the keys [0, 32 nt) of every KV head re-laid in the matrix instruction's operand order -- tile T, register v, lane (hf, li): the four floats
// K[32 T + li][32 hf + 4 v ..] -- so that a wave's request for a tile is eight instructions of 1 KiB of CONSECUTIVE bytes each. Read from the cache as it
// lies, lane (hf, li) of a request touches its own 128-byte line: 64 lines per instruction, 512 tag look-ups per tile, and eight waves of them keep a CU's
// vector cache busy for as long as the matrix pipe needs for the tile -- the first versions of k_attention_flash ran at the scratch form's speed whatever
// their inside looked like. 512 KiB per Falcon-7B launch at 2048 keys; rows beyond the cache re-read its last row. (FQ_ATTN_PACK_V: fq_attn_forms.h)
__global__ void __launch_bounds__(256) k_attn_pack_k(const float * __restrict__ kc, const float * __restrict__ vc, int N, int HKV, const int * __restrict__ n_past_ptr, float * __restrict__ kt, int nt_total) {
    const int T = blockIdx.x, hk = blockIdx.y, n_rows_cache = *n_past_ptr + N;
    f32x4 * const dst = (f32x4 *) kt + ((size_t) hk * nt_total + T) * 512;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int o = threadIdx.x + 256 * u;                          // slot of the packed tile: (v, hf, li)
        const int v = o >> 6, hf = (o >> 5) & 1, li = o & 31;
        const int j = 32 * T + li;
        dst[o] = *(const f32x4 *)(kc + ((int64_t)(j < n_rows_cache ? j : n_rows_cache - 1) * HKV + hk) * 64 + 32 * hf + 4 * v);
    }
#if FQ_ATTN_PACK_V
    // ... and the values in pass C's operand order behind all the keys: tile T, dim half dh, register quad q, lane (hf, li): V[32 T + 16 hf + 4 q + e][32 dh + li], e = 0..3 --
    // four requests of 1 KiB of consecutive bytes per tile and wave instead of sixteen that touch two 128-byte lines each
    f32x4 * const vdst = (f32x4 *)(kt + (size_t) HKV * nt_total * 2048) + ((size_t) hk * nt_total + T) * 512;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int o = threadIdx.x + 256 * u;                          // (dh, q, lane)
        const int dh = o >> 8, q = (o >> 6) & 3, hf = (o >> 5) & 1, li = o & 31;
        f32x4 t;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = 32 * T + 16 * hf + 4 * q + e;
            t[e] = vc[((int64_t)(j < n_rows_cache ? j : n_rows_cache - 1) * HKV + hk) * 64 + 32 * dh + li];
        }
        vdst[o] = t;
    }
#endif
}
// KEEP (round 5, the default up to 64 key tiles): a wave keeps the scores of ITS tiles -- T = wid, wid + 8, ...: NT / 8 tiles x 16 registers -- from pass A to pass B instead
// of running the chains twice: two units of matrix work per launch instead of three (the f32 matrix instruction and the vector ALU do not overlap on a SIMD of this
// chip, scripts/microbench/mb_mfma_f32_mix.hip: a second run of the chains is 0.18 ms of a 0.91 ms launch at 2048 tokens). The scores are the same chains' results, kept
// as c * 0.125f with the invisible ones set to -inf (table[f16(-inf)] = 0, the reference's own rule for a masked score: ggml.c:10925); pass B is then vector work only.
// LONG (round 6): contexts whose 32 rows of fp16 probabilities do NOT fit the LDS (beyond 74 key tiles = 2368 keys; the reference's 8k / 16k contexts, BASELINE
// config 5). The LDS rows hold a CHUNK of NT key tiles; the row maxima (pass A) and the row sums (pass B without stores) come from two runs of the K.Q chains over
// all tiles, then chunk after chunk: K.Q a third time -> the chunk's exp() values into LDS -> V.P of the chunk's tiles into accumulators that live across the
// chunks. Four units of f32 matrix work instead of two -- the same chains on the same operands in the same order, so the same bits as every other form
// (tests/test_gpu_block_ops.py::test_prefill_attention_forms_are_bit_identical at 4096 / 8192 / 16384 keys) -- and still no score in HBM: the scratch form
// moves N x n_kv x H x 16 bytes per launch (4.8 GB for a 512-token batch at 8192 keys) and needs a 1.2 GB scratch allocation.
template <bool TAB, int NT, bool PACKED, bool KEEP, bool LONG = false>
__global__ void __launch_bounds__(512) k_attention_flash(const float * __restrict__ qkv, int N, int H, int HKV, const int * __restrict__ n_past_ptr,
                                                         const float * __restrict__ kc, const float * __restrict__ vc,
                                                         const uint16_t * __restrict__ exp_tab, float * __restrict__ att, const float * __restrict__ kt, int nt_total, int dbg, int * __restrict__ next_item) {
    constexpr int PH = 32 * NT + 8;                                               // halfwords per LDS row (a compile-time pitch: the 16 rows of a lane are immediate offsets)
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint16_t * const eh   = (uint16_t *) smem;                                    // [32][PH] fp16 bits of exp()
    float    * const rmax = (float *)(smem + (size_t) 32 * PH * 2);               // [8 waves][32 rows]
    double   * const rsum = (double *)(rmax + 8 * 32);                            // [8 waves][32 rows]
    float    * const xch  = (float *)(rsum + 8 * 32);                             // [2 dim halves][16][64]
    const int tid = threadIdx.x, lane0 = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    // PERSISTENT workgroups (round 5): the grid is one workgroup per CU (a workgroup takes a whole CU: 8 waves x ~210 VGPRs), and each walks the (head, query tile)
    // items blockIdx.x, blockIdx.x + gridDim.x, ... -- heavy tiles (the last tokens of the prompt) first, so every workgroup gets the same mix. Per-pass timing had
    // shown 19 % of a launch to be workgroup turnover (dispatch of a 512-thread, 160 KiB workgroup onto a drained CU, kernel arguments, position word).
    // Items are handed out by a counter (next_item, zeroed by the launcher; nullptr: one item per workgroup): a fixed round-robin gave workgroups 0..70 the heaviest
    // tile of every round (512 tokens: 0.128 against 0.121 ms). The next index is fetched by one lane during the item's pass A and read by everybody behind barrier 3.
    const int n_past = *n_past_ptr;
    const int ntq = (N + 31) >> 5, n_items = ntq * H, heads = H + 2 * HKV;
    int * const nxt = (int *)(xch + 2 * 16 * 64);                     // one LDS word behind xch
  for (int item = (int) blockIdx.x; item < n_items;) {
    // (the lane's coordinates opaque per item: what the compiler derives from them -- row offsets of the output, of the value rows, LDS addresses -- is then formed in
    // the item instead of once per kernel and kept in spill slots: the registers of pass A are the kernel's peak, 224 of 256 for the scores, the queries and two key tiles)
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    const int li = lane & 31, hf = lane >> 5;
    if (next_item && tid == 64) *nxt = (int) gridDim.x + atomicAdd(next_item, 1);      // (a lane of wave 1: published by the time barrier 3 has been passed)
    const int h = item % H, i0 = (ntq - 1 - item / H) * 32, hk = h / (H / HKV);
    const int nrows = N - i0 < 32 ? N - i0 : 32;
    const int n_kv_max = n_past + i0 + nrows;                       // keys the tile's last token sees
    const int n_rows_cache = n_past + N;                            // key / value rows that exist
    const int ntile_real = (n_kv_max + 31) >> 5;
    // (tuning aid, fq_attn_switches::dbg: bits 1 / 2 / 4 run pass A / B / C over no tiles -- results are garbage, the time is what the other passes cost)
    const int ntileA = (dbg & 1) ? 0 : ntile_real, ntileB = (dbg & 2) ? 0 : ntile_real, ntileC = (dbg & 4) ? 0 : ntile_real;
    // (pass C's accumulators and roles, declared here: the LONG form runs pass C inside the scope of passes A and B, chunk by chunk)
    const int dh = wid & 1, par = (wid >> 1) & 1;
    v16f c = {0};
    // ---- passes A and B: K.Q, tiles wid, wid + 8, ...; the next tile is requested before a tile's matrix instructions start (rows beyond the cache
    // re-read its last row: every request is unconditional, the counts in the waits are exact)
    {
        f32x4 q8[8];
        const float * qrow = qkv + ((int64_t)(i0 + (li < nrows ? li : nrows - 1)) * heads + h) * 64 + 32 * hf;
#pragma unroll
        for (int v = 0; v < 8; ++v) q8[v] = ((const f32x4 *) qrow)[v];
        const float * const kbase = PACKED ? kt + (int64_t) hk * nt_total * 2048 + 4 * lane : kc + (int64_t) hk * 64 + 32 * hf;
        auto load_k = [&](int T, f32x4 (&k8)[8]) {
            if constexpr (PACKED) {                                   // (k_attn_pack_k's layout: register v of the tile is 1 KiB of consecutive bytes over the wave)
                const float * kp = kbase + (int64_t)(T < nt_total ? T : nt_total - 1) * 2048;
                const float * kq = kp + 1024;                          // (the instruction's offset field is 13 bits, signed)
                fl_gload4<0>(k8[0], kp); fl_gload4<1024>(k8[1], kp); fl_gload4<2048>(k8[2], kp); fl_gload4<3072>(k8[3], kp);
                fl_gload4<0>(k8[4], kq); fl_gload4<1024>(k8[5], kq); fl_gload4<2048>(k8[6], kq); fl_gload4<3072>(k8[7], kq);
            } else {
                const int j = 32 * T + li;
                const float * krow = kbase + (int64_t)(j < n_rows_cache ? j : n_rows_cache - 1) * HKV * 64;
                fl_gload4<0>(k8[0], krow);  fl_gload4<16>(k8[1], krow); fl_gload4<32>(k8[2], krow); fl_gload4<48>(k8[3], krow);
                fl_gload4<64>(k8[4], krow); fl_gload4<80>(k8[5], krow); fl_gload4<96>(k8[6], krow); fl_gload4<112>(k8[7], krow);
            }
        };
        f32x4 ka[8], kb[8];
        load_k(wid, ka);
        if constexpr (KEEP) {
            static_assert(FQ_FLASH_PLAIN && NT % 8 == 0, "the KEEP form uses compiler-managed loads");
            constexpr int KW = NT / 8;                                 // tiles of a wave
            v16f S[KW];
            const int tfull = (n_past + i0 + 1) >> 5;                  // tiles [0, tfull) are visible to every row of the item
#pragma unroll
            for (int k = 0; k < KW; ++k) {
                const int T = wid + 8 * k;
                if (T < ntile_real) {                                  // (wave-uniform)
                    if (k + 1 < KW) load_k(T + 8, kb);
                    v16f c = {0};
                    FL_QK(c, ka);
                    if (T < tfull) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) c[r] = c[r] * 0.125f;
                    } else {
                        const int lim = n_past + i0 - 32 * T - li;     // key 32 T + li is visible to row ir iff ir + lim >= 0
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int ir = (r & 3) + 8 * (r >> 2) + 4 * hf;
                            c[r] = (ir + lim >= 0) ? c[r] * 0.125f : -INFINITY;
                        }
                    }
                    S[k] = c;
                    if (k + 1 < KW) {
#pragma unroll
                        for (int v = 0; v < 8; ++v) ka[v] = kb[v];
                    }
                }
            }
            float mx[16];                                              // (the maxima only now: the query and key registers are free again)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx[r] = -INFINITY;
#pragma unroll
            for (int k = 0; k < KW; ++k) {
                if (wid + 8 * k < ntile_real) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) mx[r] = fq_max_f32(mx[r], S[k][r]);
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float m = reduce32(mx[r], op_max());
                if (li == 0) rmax[wid * 32 + (r & 3) + 8 * (r >> 2) + 4 * hf] = m;
            }
            __syncthreads();
            unsigned lsum[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ir = (r & 3) + 8 * (r >> 2) + 4 * hf;
                float m = rmax[ir];
#pragma unroll
                for (int w = 1; w < 8; ++w) m = fq_max_f32(m, rmax[w * 32 + ir]);
                mx[r] = m; lsum[r] = 0u;
            }
            uint16_t * const ecol = eh + (size_t)(4 * hf) * PH + li;
#pragma unroll
            for (int k = 0; k < KW; ++k) {
                const int T = wid + 8 * k;
                if (T < ntile_real) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int irl = (r & 3) + 8 * (r >> 2);
                        const uint16_t hb = f2h_bits(S[k][r] - mx[r]);
                        uint16_t eb;
                        if constexpr (TAB) eb = exp_tab[hb]; else eb = exp_f16_formula(hb);
                        ecol[irl * PH + 32 * T] = eb;
                        lsum[r] += (unsigned)(h2f_bits(eb) * 16777216.0f);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const double sm = reduce32((double) lsum[r] * (1.0 / 16777216.0), op_add());
                if (li == 0) rsum[wid * 32 + (r & 3) + 8 * (r >> 2) + 4 * hf] = sm;
            }
        } else {
        {   // pass A: row maxima
            float mx[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) mx[r] = -INFINITY;
            for (int T = wid; T < ntileA; T += 8) {
                load_k(T + 8, kb);
                FL_WAIT8(8, ka);
                __builtin_amdgcn_sched_barrier(0);                    // (the scheduler moves an asm statement wherever its operands allow: the wait for the NEXT tile went in front of this tile's matrix instructions)
                v16f c = {0};
                FL_QK(c, ka);
                const int lim = n_past + i0 - 32 * T - li;           // key 32 T + li is visible to row ir iff ir + lim >= 0
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int ir = (r & 3) + 8 * (r >> 2) + 4 * hf;
                    const float sc = c[r] * 0.125f;
                    mx[r] = fq_max_f32(mx[r], (ir < nrows && ir + lim >= 0) ? sc : -INFINITY);
                }
                __builtin_amdgcn_sched_barrier(0);
                FL_WAIT8(0, kb);                                      // (requested a whole tile of matrix instructions ago)
#pragma unroll
                for (int v = 0; v < 8; ++v) ka[v] = kb[v];
            }
            FL_WAIT8(0, ka);                                          // (a wave without tiles: its one request has landed before the registers are used for anything else)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float m = reduce32(mx[r], op_max());
                if (li == 0) rmax[wid * 32 + (r & 3) + 8 * (r >> 2) + 4 * hf] = m;
            }
        }
        load_k(wid, ka);                                              // (pass B's first tile is in flight across the barrier)
        __syncthreads();
        float mrow[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ir = (r & 3) + 8 * (r >> 2) + 4 * hf;
            float m = rmax[ir];
#pragma unroll
            for (int w = 1; w < 8; ++w) m = fq_max_f32(m, rmax[w * 32 + ir]);
            mrow[r] = m;
        }
        if constexpr (LONG) {
            static_assert(!KEEP && FQ_FLASH_PLAIN && NT % 2 == 0, "the LONG form: compiler-managed loads, whole tile pairs per chunk");
            unsigned lsum[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) lsum[r] = 0u;
            v16f cp = {0}; int Tp = 0, toff = 0;
            uint16_t * const ecol = eh + (size_t)(4 * hf) * PH + li;
            // one score of the previous tile: STORE = its exp() value into the chunk's LDS rows (tile Tp - toff of the chunk), else into the row's integer sum
            auto epiL = [&](int r, auto store_tag) {
                constexpr bool STORE = decltype(store_tag)::value;
                const int irl = (r & 3) + 8 * (r >> 2), ir = irl + 4 * hf;
                const float sc = cp[r] * 0.125f;
                const bool vis = ir < nrows && 32 * Tp + li <= n_past + i0 + ir;
                const uint16_t hb = f2h_bits(sc - mrow[r]);
                uint16_t eb;
                if constexpr (TAB) eb = exp_tab[hb]; else eb = exp_f16_formula(hb);
                eb = vis ? eb : (uint16_t) 0;
                if constexpr (STORE) ecol[irl * PH + 32 * (Tp - toff)] = eb;
                else lsum[r] += (unsigned)(h2f_bits(eb) * 16777216.0f);
            };
            // the K.Q chains of tiles Tb + wid, Tb + wid + 8, ... < Te (ka holds the first of them), pass B's software pipeline: the exp() work of a tile between the
            // matrix instructions of the next
            auto pass_b = [&](int Tb, int Te, auto store_tag) {
                if (Tb + wid < Te) {
                    load_k(Tb + wid + 8, kb);
                    v16f c0_ = {0};
                    FL_QK(c0_, ka);
                    cp = c0_; Tp = Tb + wid;
#pragma unroll
                    for (int v = 0; v < 8; ++v) ka[v] = kb[v];
                    for (int T = Tb + wid + 8; T < Te; T += 8) {
                        load_k(T + 8, kb);
                        v16f c1_ = {0};
#pragma unroll
                        for (int v = 0; v < 8; ++v) {
                            c1_ = __builtin_amdgcn_mfma_f32_32x32x2f32(q8[v].x, ka[v].x, c1_, 0, 0, 0);
                            c1_ = __builtin_amdgcn_mfma_f32_32x32x2f32(q8[v].y, ka[v].y, c1_, 0, 0, 0);
                            epiL(2 * v, store_tag);
                            __builtin_amdgcn_sched_barrier(0);
                            c1_ = __builtin_amdgcn_mfma_f32_32x32x2f32(q8[v].z, ka[v].z, c1_, 0, 0, 0);
                            c1_ = __builtin_amdgcn_mfma_f32_32x32x2f32(q8[v].w, ka[v].w, c1_, 0, 0, 0);
                            epiL(2 * v + 1, store_tag);
                            __builtin_amdgcn_sched_barrier(0);
                        }
                        cp = c1_; Tp = T;
#pragma unroll
                        for (int v = 0; v < 8; ++v) ka[v] = kb[v];
                    }
#pragma unroll
                    for (int r = 0; r < 16; ++r) epiL(r, store_tag);
                }
            };
            std::integral_constant<bool, true> STORE_T; std::integral_constant<bool, false> SUM_T;
            // ---- the row sums: every tile once more, nothing stored (a lane adds <= 64 values <= 2^24 per row at 16384 keys: exact in 32 bits)
            pass_b(0, ntileB, SUM_T);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const double sm = reduce32((double) lsum[r] * (1.0 / 16777216.0), op_add());
                if (li == 0) rsum[wid * 32 + (r & 3) + 8 * (r >> 2) + 4 * hf] = sm;
            }
            __syncthreads();
            float inv = 0.0f;
            if (wid < 4) {
                double sm = rsum[li];
#pragma unroll
                for (int w = 1; w < 8; ++w) sm += rsum[w * 32 + li];
                inv = (float)(1.0 / sm);
            }
            // ---- pass C's pieces (k_attention_flash's own, with the LDS column relative to the chunk)
            const uint16_t * erow = eh + (size_t) li * PH + 16 * hf;
            const float * const vbase = vc + (int64_t) hk * 64 + 32 * dh + li;
            const f32x4 * const vpk = (const f32x4 *)(kt + (int64_t) HKV * nt_total * 2048) + ((int64_t) hk * nt_total * 2 + dh) * 256 + lane;
            auto load_v = [&](int T, float (&v16)[16]) {
                if constexpr (PACKED && FQ_ATTN_PACK_V) {
                    const f32x4 * vp = vpk + (int64_t)(T < nt_total ? T : nt_total - 1) * 512;
#pragma unroll
                    for (int q = 0; q < 4; ++q) { const f32x4 t = vp[64 * q]; v16[4 * q] = t.x; v16[4 * q + 1] = t.y; v16[4 * q + 2] = t.z; v16[4 * q + 3] = t.w; }
                } else {
#pragma unroll
                    for (int s_ = 0; s_ < 16; ++s_) {
                        const int j = 32 * T + 16 * hf + s_;
                        fl_gload1(v16[s_], vbase + (int64_t)(j < n_rows_cache ? j : n_rows_cache - 1) * HKV * 64);
                    }
                }
            };
            auto form_p = [&](int Tl, float (&p16)[16]) {                 // Tl: the tile's index inside the chunk (one beyond the chunk reads words behind the row: never used)
                const uint4 e0 = *(const uint4 *)(erow + 32 * Tl), e1 = *(const uint4 *)(erow + 32 * Tl + 8);
                const unsigned w[8] = { e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w };
#pragma unroll
                for (int u = 0; u < 8; ++u) { p16[2 * u] = h2f_bits((uint16_t)(w[u] & 0xFFFFu)) * inv; p16[2 * u + 1] = h2f_bits((uint16_t)(w[u] >> 16)) * inv; }
            };
            auto pv_tile = [&](const float (&p16)[16], const float (&v16)[16]) {
#pragma unroll
                for (int u = 0; u < 16; ++u) c = __builtin_amdgcn_mfma_f32_32x32x2f32(p16[u], v16[u], c, 0, 0, 0);
            };
            // ---- chunk after chunk: exp() values of NT tiles into LDS, their V.P into the accumulators (tile order of a chain = ascending: the association of every form)
            for (int c0 = 0; c0 < ntile_real; c0 += NT) {
                const int c1 = c0 + NT < ntile_real ? c0 + NT : ntile_real;
                load_k(c0 + wid, ka);
                if (c0) __syncthreads();                              // (the previous chunk's pass C has read its rows)
                toff = c0;
                if (!(dbg & 2)) pass_b(c0, c1, STORE_T);
                __syncthreads();
                if (wid < 4 && !(dbg & 4)) {
                    constexpr int NB = 4;
                    float vv[NB][16], pp[2][16];
#pragma unroll
                    for (int b = 0; b < NB - 1; ++b) load_v(c0 + par + 2 * b, vv[b]);
                    int T = c0 + par;
                    form_p(T - c0, pp[0]);
                    for (; T + 2 * (NB - 1) < c1; T += 2 * NB) {
#pragma unroll
                        for (int b = 0; b < NB; ++b) {
                            load_v(T + 2 * b + 2 * (NB - 1), vv[(b + NB - 1) % NB]);
                            form_p(T - c0 + 2 * b + 2, pp[(b + 1) & 1]);
                            pv_tile(pp[b & 1], vv[b]);
                        }
                    }
#pragma unroll
                    for (int b = 0; b < NB - 1; ++b) {
                        if (T + 2 * b < c1) {
                            if (b + 1 < NB - 1) form_p(T - c0 + 2 * b + 2, pp[(b + 1) & 1]);
                            pv_tile(pp[b & 1], vv[b]);
                        }
                    }
                }
            }
            if (wid < 4 && par == 1) {
#pragma unroll
                for (int r = 0; r < 16; ++r) xch[(dh * 16 + r) * 64 + lane] = c[r];
            }
        } else
        {   // pass B: exp() values into LDS, row sums. Software-pipelined by hand: the exp() arithmetic of the wave's previous tile (~25 VALU instructions per
            // score, 16 scores per lane) is issued BETWEEN the matrix instructions of the current one -- a 64-cycle v_mfma_f32_32x32x2_f32 leaves ~14 issue
            // slots, and a wave that ran its 32 dependent matrix instructions back to back and its 400 VALU instructions after them would keep the pipe idle
            // for half of the pass. Row sums as integers: a probability's exp() is an fp16 value <= 1, i.e. k x 2^-24 with k <= 2^24, and a lane adds at most
            // ten of them per row -- exact in 32 bits (and in f64 across lanes and waves afterwards).
            unsigned lsum[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) lsum[r] = 0u;
            v16f cp = {0}; int Tp = 0;
            uint16_t * const ecol = eh + (size_t)(4 * hf) * PH + li;
            auto epi = [&](int r) {                                   // one score of the previous tile (r is a compile-time constant after unrolling)
                const int irl = (r & 3) + 8 * (r >> 2), ir = irl + 4 * hf;
                const float sc = cp[r] * 0.125f;
                const bool vis = ir < nrows && 32 * Tp + li <= n_past + i0 + ir;
                const uint16_t hb = f2h_bits(sc - mrow[r]);
                uint16_t eb;
                if constexpr (TAB) eb = exp_tab[hb]; else eb = exp_f16_formula(hb);
                eb = vis ? eb : (uint16_t) 0;
                ecol[irl * PH + 32 * Tp] = eb;
                lsum[r] += (unsigned)(h2f_bits(eb) * 16777216.0f);
            };
            if (wid < ntileB) {
                load_k(wid + 8, kb);
                FL_WAIT8(8, ka);
                __builtin_amdgcn_sched_barrier(0);
                FL_QK(cp, ka);
                Tp = wid;
                __builtin_amdgcn_sched_barrier(0);
                FL_WAIT8(0, kb);
#pragma unroll
                for (int v = 0; v < 8; ++v) ka[v] = kb[v];
                for (int T = wid + 8; T < ntileB; T += 8) {
                    load_k(T + 8, kb);
                    FL_WAIT8(8, ka);
                    __builtin_amdgcn_sched_barrier(0);
                    v16f c = {0};
#pragma unroll
                    for (int v = 0; v < 8; ++v) {
                        c = __builtin_amdgcn_mfma_f32_32x32x2f32(q8[v].x, ka[v].x, c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x2f32(q8[v].y, ka[v].y, c, 0, 0, 0);
                        epi(2 * v);
                        __builtin_amdgcn_sched_barrier(0);
                        c = __builtin_amdgcn_mfma_f32_32x32x2f32(q8[v].z, ka[v].z, c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x2f32(q8[v].w, ka[v].w, c, 0, 0, 0);
                        epi(2 * v + 1);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    cp = c; Tp = T;
                    FL_WAIT8(0, kb);
#pragma unroll
                    for (int v = 0; v < 8; ++v) ka[v] = kb[v];
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) epi(r);
            }
            FL_WAIT8(0, ka);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const double sm = reduce32((double) lsum[r] * (1.0 / 16777216.0), op_add());
                if (li == 0) rsum[wid * 32 + (r & 3) + 8 * (r >> 2) + 4 * hf] = sm;
            }
        }
        }   // !KEEP
    }
    __syncthreads();
    // ---- pass C: V.P, wave = (dim half, tile parity), waves 0-3 (one per SIMD): four chains is what the association allows. Values two tiles ahead.
    if (!LONG && wid < 4) {
        double sm = rsum[li];
#pragma unroll
        for (int w = 1; w < 8; ++w) sm += rsum[w * 32 + li];
        const float inv = (float)(1.0 / sm);
        const uint16_t * erow = eh + (size_t) li * PH + 16 * hf;
        const float * const vbase = vc + (int64_t) hk * 64 + 32 * dh + li;
        const f32x4 * const vpk = (const f32x4 *)(kt + (int64_t) HKV * nt_total * 2048) + ((int64_t) hk * nt_total * 2 + dh) * 256 + lane;      // (PACKED: k_attn_pack_k's value part)
        auto load_v = [&](int T, float (&v16)[16]) {
            if constexpr (PACKED && FQ_ATTN_PACK_V) {
                const f32x4 * vp = vpk + (int64_t)(T < nt_total ? T : nt_total - 1) * 512;
#pragma unroll
                for (int q = 0; q < 4; ++q) { const f32x4 t = vp[64 * q]; v16[4 * q] = t.x; v16[4 * q + 1] = t.y; v16[4 * q + 2] = t.z; v16[4 * q + 3] = t.w; }
            } else {
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const int j = 32 * T + 16 * hf + s;
                fl_gload1(v16[s], vbase + (int64_t)(j < n_rows_cache ? j : n_rows_cache - 1) * HKV * 64);
            }
            }
        };
        // p = e * inv, the rounding of the soft_max's own scaling step (ggml_vec_scale_f32), formed ONE TILE AHEAD of the matrix instructions that take it: the chain
        // LDS read -> convert -> multiply -> matrix instruction was exposed twice per tile (ds_read_b128, s_waitcnt lgkmcnt(0), 8 matrix instructions) -- a fifth of the
        // pass; with the next tile's sixteen values formed between this tile's matrix instructions only their issue slots are left
        auto form_p = [&](int T, float (&p16)[16]) {
            const uint4 e0 = *(const uint4 *)(erow + 32 * T), e1 = *(const uint4 *)(erow + 32 * T + 8);
            const unsigned w[8] = { e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w };
#pragma unroll
            for (int u = 0; u < 8; ++u) { p16[2 * u] = h2f_bits((uint16_t)(w[u] & 0xFFFFu)) * inv; p16[2 * u + 1] = h2f_bits((uint16_t)(w[u] >> 16)) * inv; }
        };
        auto pv_tile = [&](const float (&p16)[16], const float (&v16)[16]) {
#pragma unroll
            for (int u = 0; u < 16; ++u) c = __builtin_amdgcn_mfma_f32_32x32x2f32(p16[u], v16[u], c, 0, 0, 0);
        };
        constexpr int NB = 4;                                           // value tiles T, T + 2, T + 4, T + 6 of this parity in flight (even: the p buffers alternate)
        float vv[NB][16], pp[2][16];
#pragma unroll
        for (int b = 0; b < NB - 1; ++b) load_v(par + 2 * b, vv[b]);
        int T = par;
        form_p(T, pp[0]);                                               // (a tile index beyond the item's last reads LDS words behind the row: never used)
        for (; T + 2 * (NB - 1) < ntileC; T += 2 * NB) {
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                load_v(T + 2 * b + 2 * (NB - 1), vv[(b + NB - 1) % NB]);
                form_p(T + 2 * b + 2, pp[(b + 1) & 1]);
                pv_tile(pp[b & 1], vv[b]);
            }
        }
#pragma unroll
        for (int b = 0; b < NB - 1; ++b) {
            if (T + 2 * b < ntileC) {
                if (b + 1 < NB - 1) form_p(T + 2 * b + 2, pp[(b + 1) & 1]);
                pv_tile(pp[b & 1], vv[b]);
            }
        }
        if (par == 1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) xch[(dh * 16 + r) * 64 + lane] = c[r];
        }
    }
    __syncthreads();
    if (wid < 2) {                                                      // par == 0: E + O
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ir = (r & 3) + 8 * (r >> 2) + 4 * hf;
            if (ir < nrows) att[(int64_t)(i0 + ir) * H * 64 + (int64_t) h * 64 + 32 * dh + li] = c[r] + xch[(dh * 16 + r) * 64 + lane];
        }
    }
    // (no barrier before the next item: its first LDS writes are rmax after its pass A -- a region nobody reads now --, eh / rsum / xch only behind its own barriers;
    // the next index word is rewritten by wave 1 only after wave 1 itself has read it, and every other wave reads it before its next barrier 1)
    item = next_item ? __builtin_amdgcn_readfirstlane(*(volatile int *) nxt) : n_items;      // (wave-uniform, and known to the compiler as such: the item's tile counts and row bases stay scalar)
    if (next_item) __syncthreads();                                   // (the word is rewritten at the top of the next item: everybody must have read it)
  }
}

// ------------------------------------------------------------------------------------------------ the launcher
static int g_attn_f64 = 0;
static int g_attn_form = 0;      // prefill attention on the matrix pipe (fq_attn_mode::form): 0 = default, 1 = k_attention_flash, 32 = k_attention_mfma, 16 = k_attention_mfma16, 17 = k_attention_mfma16h
void fq_attn_set_form(int form) { g_attn_form = form; }
void fq_attn_set_f64(int on) { g_attn_f64 = on != 0; }
int  fq_attn_f64() { return g_attn_f64; }
static fq_attn_mode attn_mode_now() { return fq_attn_mode_of(g_attn_f64 != 0, g_attn_form, fq_attn_sw()); }
size_t fq_attention_scratch_need(int N, int H, int max_n_kv, int HKV) { return fq_attn_scratch_need(N, H, max_n_kv, HKV, fq_attn_sw()); }
void fq_attn_plan_debug(int N, int H, int HKV, int D, int max_n_kv, int64_t * out) {
    fq_attn_plan_ints(fq_attn_plan_of(N, H, HKV, D, max_n_kv, false, attn_mode_now(), fq_attn_sw(), fq_ctx().n_cu, fq_attn_scratch_cap(fq_attn_sw())), out);
}

// score rows / packed keys of long-context launches. A model context owns its own buffer, sized once for its (n_batch, n_ctx) at context_create
// (fq_attention_scratch_need) and passed in; the process-wide one below serves only the op-level API (ggml_hip_attention: synchronous, one stream) and is grown on
// demand up to fq_attn_scratch_cap(). The plan asks for no more than either can hold; nullptr: the process-wide allocation failed.
static float * g_att_scratch = nullptr;
static size_t  g_att_scratch_bytes = 0;
static float * att_scratch(fq_att_scratch * own, size_t bytes, hipStream_t st) {
    if (own) return bytes <= own->bytes ? own->p : nullptr;          // never grown here: launches of a context may be captured
    if (bytes > g_att_scratch_bytes) {
        HIP_CHECK(hipStreamSynchronize(st));
        if (g_att_scratch) HIP_CHECK(hipFree(g_att_scratch));
        g_att_scratch = nullptr; g_att_scratch_bytes = 0;
        if (hipMalloc((void **) &g_att_scratch, bytes) != hipSuccess) { (void) hipGetLastError(); g_att_scratch = nullptr; return nullptr; }
        g_att_scratch_bytes = bytes;
    }
    return g_att_scratch;
}

// what every kernel of the prompt attention is handed
struct attn_args { const float * qkv; int N, H, HKV; const int * n_past; const float * kc, * vc; const uint16_t * exp_tab; float * att; };

template <int R>
static void launch_attention_rows(const fq_attn_plan & p, const attn_args & a, float * scr, hipStream_t st) {
    if (g_attn_f64) {
        attn_grant_lds<&k_attention_rows<R, true>>(p.lds);
        hipLaunchKernelGGL((k_attention_rows<R, true>), dim3(p.grid_x, p.grid_y), dim3(p.block), p.lds, st, a.qkv, a.N, a.H, a.HKV, a.n_past, a.kc, a.vc, a.exp_tab, a.att, p.pitch, scr);
    } else {
        attn_grant_lds<&k_attention_rows<R, false>>(p.lds);
        hipLaunchKernelGGL((k_attention_rows<R, false>), dim3(p.grid_x, p.grid_y), dim3(p.block), p.lds, st, a.qkv, a.N, a.H, a.HKV, a.n_past, a.kc, a.vc, a.exp_tab, a.att, p.pitch, scr);
    }
}
// k_attention_flash: <NT, KEEP, LONG> from the plan; TAB = there is an exp table; PACKED = kt holds the re-laid keys and values
template <bool TAB, int NT, bool PACKED, bool KEEP, bool LONG>
static void launch_attention_flash_t(const fq_attn_plan & p, const attn_args & a, const float * kt, hipStream_t st) {
    attn_grant_lds<&k_attention_flash<TAB, NT, PACKED, KEEP, LONG>>(p.lds);
    int * counter = p.persistent ? fq_ctx().scalar_i32 + 32 : nullptr;           // (a word of the library's scalar scratch; zeroed on the launch's own stream)
    if (counter) HIP_CHECK(hipMemsetAsync(counter, 0, 4, st));
    hipLaunchKernelGGL((k_attention_flash<TAB, NT, PACKED, KEEP, LONG>), dim3(p.grid_x), dim3(p.block), p.lds, st, a.qkv, a.N, a.H, a.HKV, a.n_past, a.kc, a.vc, a.exp_tab, a.att, kt, p.nt_total, p.dbg, counter);
}
template <int NT, bool KEEP, bool LONG>
static void launch_attention_flash(const fq_attn_plan & p, const attn_args & a, const float * kt, hipStream_t st) {
    if (a.exp_tab) { if (p.packed) launch_attention_flash_t<true, NT, true, KEEP, LONG>(p, a, kt, st);  else launch_attention_flash_t<true, NT, false, KEEP, LONG>(p, a, kt, st); }
    else           { if (p.packed) launch_attention_flash_t<false, NT, true, KEEP, LONG>(p, a, kt, st); else launch_attention_flash_t<false, NT, false, KEEP, LONG>(p, a, kt, st); }
}

void fq_launch_attention(const float * qkv, int N, int H, int HKV, int D, const int * n_past_dev, int max_n_kv, const float * k_cache,
                         const float * v_cache, const uint16_t * exp_table, float * att, hipStream_t st, int64_t seq_stride, fq_att_scratch * own_scratch,
                         int pos_stride) {
    FQ_TL(st, "attention");
    const fq_attn_switches & sw = fq_attn_sw();
    const fq_attn_mode mode = attn_mode_now();
    auto plan_with = [&](size_t cap) { return fq_attn_plan_of(N, H, HKV, D, max_n_kv, seq_stride != 0, mode, sw, fq_ctx().n_cu, cap); };
    fq_attn_plan p = plan_with(own_scratch ? own_scratch->bytes : fq_attn_scratch_cap(sw));
    float * scr = p.scratch_bytes ? att_scratch(own_scratch, p.scratch_bytes, st) : nullptr;
    if (p.scratch_bytes && !scr) { p = plan_with(g_att_scratch_bytes); scr = p.scratch_bytes ? g_att_scratch : nullptr; }      // the process-wide allocation failed: what it holds now (nothing)
    attn_args a = { qkv, N, H, HKV, n_past_dev, k_cache, v_cache, exp_table, att };
    switch (p.family) {
    case FQ_AF_REFUSE_HEAD_DIM: fprintf(stderr, "ggml-hip: attention: head_dim %d != 64\n", D); exit(1);
    case FQ_AF_REFUSE_KEYS:     fprintf(stderr, "ggml-hip: attention: %d keys do not fit the score buffer in LDS\n", max_n_kv); exit(1);
    case FQ_AF_FLASH:
        if (!a.exp_tab && p.ctx_tab) a.exp_tab = fq_ctx().exp_table;
        if (p.packed) hipLaunchKernelGGL(k_attn_pack_k, dim3((unsigned) p.nt_total, (unsigned) HKV), dim3(256), 0, st, k_cache, v_cache, N, HKV, n_past_dev, scr, p.nt_total);
        switch (p.nt * 4 + p.keep * 2 + p.lng) {       // (the instantiations that exist: fq_attn_flash_pitch_of gives no other)
        case 16 * 4 + 2: launch_attention_flash<16, true, false>(p, a, scr, st);  break;
        case 16 * 4:     launch_attention_flash<16, false, false>(p, a, scr, st); break;
        case 32 * 4 + 2: launch_attention_flash<32, true, false>(p, a, scr, st);  break;
        case 32 * 4:     launch_attention_flash<32, false, false>(p, a, scr, st); break;
        case 64 * 4 + 2: launch_attention_flash<64, true, false>(p, a, scr, st);  break;
        case 64 * 4 + 1: launch_attention_flash<64, false, true>(p, a, scr, st);  break;
        default:         launch_attention_flash<74, false, false>(p, a, scr, st); break;
        }
        break;
    case FQ_AF_MFMA16:
        attn_grant_lds<&k_attention_mfma16>(p.lds);
        hipLaunchKernelGGL(k_attention_mfma16, dim3(p.grid_x, p.grid_y), dim3(p.block), p.lds, st, qkv, N, H, HKV, n_past_dev, k_cache, v_cache, exp_table, att, p.pitch);
        break;
    case FQ_AF_MFMA16H:
        attn_grant_lds<&k_attention_mfma16h>(p.lds);
        hipLaunchKernelGGL(k_attention_mfma16h, dim3(p.grid_x, p.grid_y), dim3(p.block), p.lds, st, qkv, N, H, HKV, n_past_dev, k_cache, v_cache, exp_table, att, p.pitch);
        break;
    case FQ_AF_MFMA_SCRATCH:
        hipLaunchKernelGGL(k_attention_mfma, dim3(p.grid_x, p.grid_y), dim3(p.block), 0, st, qkv, N, H, HKV, n_past_dev, k_cache, v_cache, exp_table, att, p.pitch, scr);
        break;
    case FQ_AF_ROWS_SCRATCH: launch_attention_rows<4>(p, a, scr, st); break;
    case FQ_AF_ROWS_LDS:
        if (p.R == 8) launch_attention_rows<8>(p, a, nullptr, st); else if (p.R == 4) launch_attention_rows<4>(p, a, nullptr, st); else launch_attention_rows<2>(p, a, nullptr, st);
        break;
    default: {     // FQ_AF_ONE_ROW
        attn_grant_lds<&k_attention<false>>(p.lds); attn_grant_lds<&k_attention<true>>(p.lds);
        const int ps = seq_stride ? pos_stride : 0;
        if (g_attn_f64) hipLaunchKernelGGL(k_attention<true>, dim3(p.grid_x, p.grid_y), dim3(p.block), p.lds, st, qkv, H, HKV, n_past_dev, k_cache, v_cache, exp_table, att, seq_stride, ps);
        else            hipLaunchKernelGGL(k_attention<false>, dim3(p.grid_x, p.grid_y), dim3(p.block), p.lds, st, qkv, H, HKV, n_past_dev, k_cache, v_cache, exp_table, att, seq_stride, ps);
    } }
}

// ------------------------------------------------------------------------------------------------ draft-and-verify passes
// The N rows of a verify pass (falcon_hip_decode_spec) are N consecutive positions of ONE cache, n_past + t -- a prompt batch -- but the pass always has N
// rows, also where fewer fit: a row whose position would be >= limit (the cache's length) appends nothing, reads no rope row, and its attention output is
// zeros (its logits are never looked at: fq_spec.h's fq_spec_go_on). Everything else is k_rope_kv and k_attention at seq_stride 0, beside which these stand.
// Row t attends to the keys [0, n_past + t], those of rows < t among them: the append is a launch of its own in front of the attention's.
__global__ void k_rope_kv_lim(float * __restrict__ qkv, int N, int H, int HKV, int D, const int * __restrict__ n_past_ptr, const float * __restrict__ cs,
                              float * __restrict__ kc, float * __restrict__ vc, int limit) {
    const int half = D >> 1;
    const int heads = H + 2 * HKV;
    const int n_past = *n_past_ptr;
    const int64_t total = (int64_t) N * heads * half;
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t) gridDim.x * blockDim.x) {
        const int k = (int)(i % half);
        const int h = (int)((i / half) % heads);
        const int t = (int)(i / ((int64_t) half * heads));
        const int pos = n_past + t;
        if (pos >= limit) continue;
        float * v = qkv + ((int64_t) t * heads + h) * D;
        if (h < H + HKV) {
            const float c = cs[((int64_t) pos * half + k) * 2], s = cs[((int64_t) pos * half + k) * 2 + 1];
            const float x0 = v[k], x1 = v[k + half];
            const float r0 = x0 * c - x1 * s, r1 = x0 * s + x1 * c;     // ggml.c:12974-12975
            if (h < H) { v[k] = r0; v[k + half] = r1; }
            else { float * o = kc + ((int64_t) pos * HKV + (h - H)) * D; o[k] = r0; o[k + half] = r1; }
        } else {
            float * o = vc + ((int64_t) pos * HKV + (h - H - HKV)) * D;
            o[k] = v[k]; o[k + half] = v[k + half];
        }
    }
}
template <bool F64>
__global__ void __launch_bounds__(256) k_attention_lim(const float * __restrict__ qkv, int H, int HKV, const int * __restrict__ n_past_ptr,
                                                       const float * __restrict__ kc, const float * __restrict__ vc,
                                                       const uint16_t * __restrict__ exp_tab, float * __restrict__ att, int limit) {
    constexpr int D = 64;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int h = blockIdx.x, t = blockIdx.y;
    const int n_kv = *n_past_ptr + t + 1;
    if (n_kv > limit) {                                     // (block-uniform)
        if (threadIdx.x < 64) att[(int64_t) t * H * D + (int64_t) h * D + threadIdx.x] = 0.0f;
        return;
    }
    const int heads = H + 2 * HKV;
    const int hk = h / (H / HKV);
    const attn_lds L = attn_lds_carve(smem);
    const float o = attn_head_block<F64>(qkv + ((int64_t) t * heads + h) * D, kc, vc, HKV, hk, n_kv, nullptr, nullptr, exp_tab, L);
    if (threadIdx.x < 64) att[(int64_t) t * H * D + (int64_t) h * D + threadIdx.x] = o;
}
// limit keys at the most: the score row in LDS is sized for them. false (nothing launched): they do not fit it
bool fq_verify_attention_fits(int limit) { return fq_attn_one_row_fits(limit); }
void fq_launch_rope_kv_verify(float * qkv, int N, int H, int HKV, int D, const int * n_past_dev, int limit, const float * rope_cs, float * k_cache, float * v_cache, hipStream_t st) {
    FQ_TL(st, "rope_kv");
    const int64_t total = (int64_t) N * (H + 2 * HKV) * (D / 2);
    const int blocks = (int) ((total + 255) / 256 > 8192 ? 8192 : (total + 255) / 256);
    hipLaunchKernelGGL(k_rope_kv_lim, dim3(blocks), dim3(256), 0, st, qkv, N, H, HKV, D, n_past_dev, rope_cs, k_cache, v_cache, limit);
}
void fq_launch_attention_verify(const float * qkv, int N, int H, int HKV, int D, const int * n_past_dev, int limit, const float * k_cache, const float * v_cache,
                                const uint16_t * exp_table, float * att, hipStream_t st) {
    FQ_TL(st, "attention");
    if (D != 64 || !fq_verify_attention_fits(limit)) { fprintf(stderr, "ggml-hip: verify attention: head_dim %d != 64, or %d keys do not fit the score buffer in LDS\n", D, limit); exit(1); }
    const size_t lds = fq_attn_one_row_lds(limit);
    attn_grant_lds<&k_attention_lim<false>>(lds); attn_grant_lds<&k_attention_lim<true>>(lds);
    if (g_attn_f64) hipLaunchKernelGGL(k_attention_lim<true>, dim3((unsigned) H, (unsigned) N), dim3(256), lds, st, qkv, H, HKV, n_past_dev, k_cache, v_cache, exp_table, att, limit);
    else            hipLaunchKernelGGL(k_attention_lim<false>, dim3((unsigned) H, (unsigned) N), dim3(256), lds, st, qkv, H, HKV, n_past_dev, k_cache, v_cache, exp_table, att, limit);
}

