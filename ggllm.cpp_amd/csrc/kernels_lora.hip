// kernels_lora.hip -- the device side of a LoRA merge (fq_lora.h: the file; falcon_model.hip: the chunk pipeline) for gfx950, wave64.
//
//  * k_lora_add   the reference's low-rank product, element by element as its scalar build computes it (llama_apply_lora_from_file_internal,
//                 libfalcon.cpp:4127-4142: mul_mat(loraA, loraB) -> scale -> add), for a chunk of rows of one matrix:
//                   1. s is a double that starts at 0; for i = 0 .. r-1 IN THAT ORDER  s += (double)(float)(A[k][i] * B[m][i])     (ggml_vec_dot_f32, ggml.c:2296-2300;
//                      F16 loraA: ggml_vec_dot_f16 over fp16(B) -- the caller widens both to f32 first, the f32 product of two fp16 values is exact)
//                      ba = (float) s
//                   2. scaling != 1: ba = ba * scaling                                                                                (ggml_vec_scale_f32)
//                   3. f32 staging row: x = x + ba;  F16 row: w = fp16(fp32(w) + ba)                                                  (ggml.c:8599-8626, 8457-8459)
//                 Every rounding is spelled out (__fmul_rn, __dadd_rn, __fadd_rn): nothing here may contract into an FMA. One thread owns one element's whole
//                 chain -- no cross-lane reduction, the order is the contract. A workgroup takes 256 consecutive columns k (lane = column: the staging row's
//                 loads and stores coalesce) and walks rows; its 256 rows of A sit in LDS when r allows (rows r|1 floats apart: the lanes' reads of their own
//                 rows spread over the banks), else they are read through the cache. B[m][i] is the same address for the whole workgroup.
//                 Not tuned beyond that: nothing in it has been measured against a variant.
//  * k_untile     the inverse of k_retile (kernels_quant.hip): the interleaved planes of rows back into ggml's array of blocks (falcon_hip_model_get_tensor)
#include "fq_device.h"
#include "fq_f16.h"
#include "kernels.h"

#define LORA_TK 256                          // columns per workgroup = threads
#define LORA_LDS_MAX_R 40                    // A tile in LDS up to this r: 256 x 41 floats = 41 KiB

template <bool LDS, bool F16DST>
__global__ void __launch_bounds__(LORA_TK) k_lora_add(const float * __restrict__ A, const float * __restrict__ B, int r, int64_t K, int64_t nrows, float scaling,
                                                      int scale_on, void * __restrict__ dst, int64_t ldd) {
    extern __shared__ float s_a[];
    const int64_t k0 = (int64_t) blockIdx.x * LORA_TK, k = k0 + threadIdx.x;
    const int rp = r | 1;
    if (LDS) {
        const int64_t ncol = K - k0 < LORA_TK ? K - k0 : LORA_TK;
        for (int64_t j = threadIdx.x; j < ncol * r; j += LORA_TK) {          // consecutive floats of A: coalesced
            const int c = (int)(j / r), i = (int)(j - (int64_t) c * r);
            s_a[c * rp + i] = A[k0 * r + j];
        }
        __syncthreads();
    }
    if (k >= K) return;
    const float * a = LDS ? s_a + threadIdx.x * rp : A + k * r;
    for (int64_t m = blockIdx.y; m < nrows; m += gridDim.y) {
        const float * b = B + m * r;
        double s = 0.0;
        for (int i = 0; i < r; ++i) s = __dadd_rn(s, (double) __fmul_rn(a[i], b[i]));
        float ba = (float) s;
        if (scale_on) ba = __fmul_rn(ba, scaling);
        if (F16DST) {
            uint16_t * w = (uint16_t *) dst + m * ldd + k;
            *w = fq_f32_to_f16_bits(__fadd_rn(fq_f16_bits_to_f32(*w), ba));
        } else {
            float * x = (float *) dst + m * ldd + k;
            *x = __fadd_rn(*x, ba);
        }
    }
}

// dst rows [0, nrows) += scaling * (B rows [0, nrows)) . A^T; A [K][r], B [nrows][r] f32 on the device. dst: f32 rows (dst_f16 false) or fp16 rows, ldd elements apart
void fq_launch_lora_add(const float * A, const float * B, int r, int64_t K, int64_t nrows, float scaling, void * dst, int64_t ldd, bool dst_f16, hipStream_t st) {
    FQ_TL(st, "lora_add");
    if (nrows <= 0 || K <= 0 || r <= 0) return;
    const unsigned gx = (unsigned)((K + LORA_TK - 1) / LORA_TK);
    int64_t gy = nrows;
    const int64_t cap = 65535 < (int64_t) 16384 / gx + 1 ? 65535 : (int64_t) 16384 / gx + 1;      // enough workgroups to fill the chip, each re-using its A tile over its rows
    if (gy > cap) gy = cap;
    const dim3 grid(gx, (unsigned) gy);
    const int scale_on = scaling != 1.0f ? 1 : 0;                                                 // (libfalcon.cpp:4130)
    const bool lds = r <= LORA_LDS_MAX_R;
    const size_t sh = lds ? (size_t) LORA_TK * (size_t)(r | 1) * 4 : 0;
    if (lds && dst_f16)       hipLaunchKernelGGL((k_lora_add<true, true>),   grid, dim3(LORA_TK), sh, st, A, B, r, K, nrows, scaling, scale_on, dst, ldd);
    else if (lds)             hipLaunchKernelGGL((k_lora_add<true, false>),  grid, dim3(LORA_TK), sh, st, A, B, r, K, nrows, scaling, scale_on, dst, ldd);
    else if (dst_f16)         hipLaunchKernelGGL((k_lora_add<false, true>),  grid, dim3(LORA_TK), sh, st, A, B, r, K, nrows, scaling, scale_on, dst, ldd);
    else                      hipLaunchKernelGGL((k_lora_add<false, false>), grid, dim3(LORA_TK), sh, st, A, B, r, K, nrows, scaling, scale_on, dst, ldd);
}

// ------------------------------------------------------------------------------------------------ un-tile
__global__ void k_untile(fq_weight w, int type, uint8_t * __restrict__ dst) {
    const fq_type_desc d = fq_desc(type);
    const int64_t total = w.M * w.nblk;
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t) gridDim.x * blockDim.x) {
        uint8_t * o = dst + (size_t) i * d.tsize;
        const int64_t row = i / w.nblk, blk = i - row * w.nblk;
        for (int p = 0; p < d.nplanes; ++p) {
            const uint8_t * s = w.plane[0] + (size_t) row * w.row_stride + fq_il_offset(d, p, w.nblk, blk);
            for (int b = 0; b < d.plane[p].bytes; ++b) o[d.plane[p].src_off + b] = s[b];
        }
    }
}

// rows [0, w.M) of a quantized matrix as ggml blocks at dst_dev (w.M * w.nblk * tsize bytes)
void fq_launch_untile(const fq_weight & w, uint8_t * dst_dev, hipStream_t st) {
    FQ_TL(st, "untile");
    const int64_t total = w.M * w.nblk;
    if (total <= 0) return;
    const int blocks = (int) ((total + 255) / 256 > 8192 ? 8192 : (total + 255) / 256);
    hipLaunchKernelGGL(k_untile, dim3(blocks), dim3(256), 0, st, w, w.type, dst_dev);
}
