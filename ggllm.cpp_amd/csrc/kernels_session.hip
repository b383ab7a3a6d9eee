// kernels_session.hip -- a sequence's K and V rows between the cache and a contiguous staging buffer in the session file's layout (fq_session.h):
//   cache    K, V  f32 [layer][row][R]               R = n_head_kv * 64; a sequence's rows start at first_row, layers lie layer_pitch rows apart
//   staging  K     f32 [layer][n_tok][R]             as it lies
//            V     f32 [layer][R][n_tok]             transposed (the reference keeps V that way: libfalcon.cpp:2256-2280, 4303, 4324-4328)
// One launch each way, grid (tiles, layers, K | V) like k_copy_seq_kv. The K half streams float4 (R is a multiple of 64, so every layer of either
// side begins on 256 bytes). The V half moves 64 positions x 64 dims per workgroup through LDS: the cache side runs along dims, the staging side along
// positions, either way one wave row is 64 consecutive floats = 256 bytes. The tile's row pitch is 65 floats: the accesses are 32-bit, whose bank is
// (byte / 4) % 32 counted per 32-lane half -- along a tile row the 32 lanes of a half sit on 32 consecutive words (32 banks, any pitch), down a tile
// column on words 65 apart = banks 1 apart (32 banks; a pitch of 64 would put the whole half on ONE bank, any even pitch on at most 16).
// n_tok need not be a multiple of anything: partial tiles are masked, and the staging V rows start at any word, so that side moves single floats.
// All offsets are 64-bit (Falcon-40B at 2048 keys: 252 MB per tensor).
#include "fq_device.h"
#include "kernels.h"
#include "hip_context.h"
#include "../../include/ggml-hip-ops.h"

#define FQ_SS_TILE 64
#define FQ_SS_PITCH 65
#define FQ_SS_THREADS 256

// UNPACK false: cache -> staging; true: staging -> cache (cache rows [first, first + n_tok) of every layer, nothing else)
template <bool UNPACK>
__device__ __forceinline__ void session_move(float * __restrict__ kc, float * __restrict__ vc, float * __restrict__ stage, int n_head_kv, int n_tok,
                                             int64_t layer_pitch /* floats */, float * tile) {
    const int64_t R = (int64_t) n_head_kv * 64, layer = blockIdx.y;
    const int64_t per_layer = (int64_t) n_tok * R;                 // floats of one layer in the staging buffer, K or V
    if (blockIdx.z == 0) {                                         // K: the rows as they lie
        float4 * c = (float4 *)(kc + layer * layer_pitch);
        float4 * s = (float4 *)(stage + layer * per_layer);
        const int64_t n4 = per_layer / 4;
        for (int64_t i = (int64_t) blockIdx.x * FQ_SS_THREADS + threadIdx.x; i < n4; i += (int64_t) gridDim.x * FQ_SS_THREADS) {
            if (UNPACK) c[i] = s[i]; else s[i] = c[i];
        }
        return;
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;       // 4 waves, 16 tile rows each
    const int64_t p0 = (int64_t)(blockIdx.x / n_head_kv) * FQ_SS_TILE;
    const int64_t d0 = (int64_t)(blockIdx.x % n_head_kv) * FQ_SS_TILE;
    float * c = vc + layer * layer_pitch + d0;                     // [pos][R], this tile's 64 dims
    float * s = stage + ((int64_t) gridDim.y + layer) * per_layer + d0 * n_tok;      // V lies behind all of K: [dim][n_tok]
    if (!UNPACK) {
        for (int i = 0; i < FQ_SS_TILE / 4; ++i) {                 // cache rows: lane = dim
            const int p = w + 4 * i;
            if (p0 + p < n_tok) tile[p * FQ_SS_PITCH + lane] = c[(p0 + p) * R + lane];
        }
        __syncthreads();
        if (p0 + lane < n_tok)
            for (int i = 0; i < FQ_SS_TILE / 4; ++i) {             // staging rows: lane = position
                const int d = w + 4 * i;
                s[(int64_t) d * n_tok + p0 + lane] = tile[lane * FQ_SS_PITCH + d];
            }
    } else {
        if (p0 + lane < n_tok)
            for (int i = 0; i < FQ_SS_TILE / 4; ++i) {
                const int d = w + 4 * i;
                tile[lane * FQ_SS_PITCH + d] = s[(int64_t) d * n_tok + p0 + lane];
            }
        __syncthreads();
        for (int i = 0; i < FQ_SS_TILE / 4; ++i) {
            const int p = w + 4 * i;
            if (p0 + p < n_tok) c[(p0 + p) * R + lane] = tile[p * FQ_SS_PITCH + lane];
        }
    }
}

__global__ void __launch_bounds__(FQ_SS_THREADS) k_session_pack(const float * __restrict__ kc, const float * __restrict__ vc, float * __restrict__ stage,
                                                                int n_head_kv, int n_tok, int64_t layer_pitch) {
    __shared__ float tile[FQ_SS_TILE * FQ_SS_PITCH];
    session_move<false>((float *) kc, (float *) vc, stage, n_head_kv, n_tok, layer_pitch, tile);
}
__global__ void __launch_bounds__(FQ_SS_THREADS) k_session_unpack(float * __restrict__ kc, float * __restrict__ vc, const float * __restrict__ stage,
                                                                  int n_head_kv, int n_tok, int64_t layer_pitch) {
    __shared__ float tile[FQ_SS_TILE * FQ_SS_PITCH];
    session_move<true>(kc, vc, (float *) stage, n_head_kv, n_tok, layer_pitch, tile);
}

static bool session_args_ok(const char * what, const void * k, const void * v, const void * stage, int n_layer, int n_head_kv, int n_tok,
                            int64_t layer_pitch_rows, int64_t first_row) {
    const int64_t tiles = ((int64_t) n_tok + FQ_SS_TILE - 1) / FQ_SS_TILE * (int64_t) n_head_kv;
    if (!k || !v || !stage || n_layer < 1 || n_layer > 65535 || n_head_kv < 1 || n_tok < 0 || first_row < 0 || layer_pitch_rows < first_row + n_tok ||
        tiles > 0x7fffffff) {
        fprintf(stderr, "ggml-hip: %s: bad arguments (%d layers, %d kv heads, %d rows from row %lld, %lld rows between layers)\n", what, n_layer, n_head_kv,
                n_tok, (long long) first_row, (long long) layer_pitch_rows);
        return false;
    }
    return true;
}

template <bool UNPACK>
static void session_launch(float * k, float * v, float * stage, int n_layer, int n_head_kv, int n_tok, int64_t layer_pitch_rows, int64_t first_row, hipStream_t st) {
    if (n_tok == 0) return;
    const int64_t R = (int64_t) n_head_kv * 64;
    const unsigned tiles = (unsigned)(((int64_t) n_tok + FQ_SS_TILE - 1) / FQ_SS_TILE * n_head_kv);
    const dim3 grid(tiles, (unsigned) n_layer, 2);
    if (UNPACK) hipLaunchKernelGGL(k_session_unpack, grid, dim3(FQ_SS_THREADS), 0, st, k + first_row * R, v + first_row * R, (const float *) stage, n_head_kv, n_tok, layer_pitch_rows * R);
    else        hipLaunchKernelGGL(k_session_pack, grid, dim3(FQ_SS_THREADS), 0, st, (const float *)(k + first_row * R), (const float *)(v + first_row * R), stage, n_head_kv, n_tok, layer_pitch_rows * R);
}

void fq_launch_session_pack(const float * k_cache, const float * v_cache, float * staging, int n_layer, int n_head_kv, int n_tok,
                            int64_t layer_pitch_rows, int64_t first_row, hipStream_t st) {
    session_launch<false>((float *) k_cache, (float *) v_cache, staging, n_layer, n_head_kv, n_tok, layer_pitch_rows, first_row, st);
}
void fq_launch_session_unpack(float * k_cache, float * v_cache, const float * staging, int n_layer, int n_head_kv, int n_tok,
                              int64_t layer_pitch_rows, int64_t first_row, hipStream_t st) {
    session_launch<true>(k_cache, v_cache, (float *) staging, n_layer, n_head_kv, n_tok, layer_pitch_rows, first_row, st);
}

extern "C" int ggml_hip_kv_pack(const float * k_cache_dev, const float * v_cache_dev, float * staging_dev, int n_layer, int n_head_kv, int n_tok,
                                int64_t layer_pitch_rows, int64_t first_row) {
    if (!session_args_ok("kv_pack", k_cache_dev, v_cache_dev, staging_dev, n_layer, n_head_kv, n_tok, layer_pitch_rows, first_row)) return 1;
    fq_launch_session_pack(k_cache_dev, v_cache_dev, staging_dev, n_layer, n_head_kv, n_tok, layer_pitch_rows, first_row, fq_ctx().stream);
    return 0;
}
extern "C" int ggml_hip_kv_unpack(float * k_cache_dev, float * v_cache_dev, const float * staging_dev, int n_layer, int n_head_kv, int n_tok,
                                  int64_t layer_pitch_rows, int64_t first_row) {
    if (!session_args_ok("kv_unpack", k_cache_dev, v_cache_dev, staging_dev, n_layer, n_head_kv, n_tok, layer_pitch_rows, first_row)) return 1;
    fq_launch_session_unpack(k_cache_dev, v_cache_dev, staging_dev, n_layer, n_head_kv, n_tok, layer_pitch_rows, first_row, fq_ctx().stream);
    return 0;
}
