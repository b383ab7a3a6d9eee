// fq_mm_forms.h -- which kernel form a quantized mat-mul takes: ONE statement of the rules, as pure functions of the matrix (type, rows, blocks per row), the
// number of columns N, the chip's CUs, the process modes and the environment switches. No HIP in here: g++ compiles it for tests/host/mm_forms_harness.cpp
// (tests/test_mm_forms_cpu.py pins the table). The launchers (fq_launch_gemm, fq_launch_gemm_skinny*, fq_mul_mat_q_acts*) and whoever asks "would it?"
// (launch_stage's two-stream and column rules) run THIS code; the launchers that return bool keep their refusals as a backstop.
// The measured numbers behind every threshold stand next to the rule they justify.
#pragma once
#include "fq_types.h"
#include <stdlib.h>
#include <initializer_list>

// ---- constants the rules share with the kernels (the kernel files static_assert their own against these)
#define FQ_GEMV_MAX_COLS 4                                 // the column mat-vec serves up to 4 columns per weight pass (kernels_gemv.hip)
#define FQ_KS_MAX_M 32768                                  // rows of the legacy K-share form's partial-sum scratch
#define FQ_KS_FLOATS ((size_t) 16 << 20)                   // the scratch: 64 MiB = [segment][share][16 columns][rows] of the k-quant forms (4 x 16 x FQ_KS_MAX_M of the legacy K-share form)
#define FQ_SKINNY_Q4K_MAX_COLS 112                         // the k-quants' streaming forms in passes of 16, at most (fq_skinny_kq_max_cols(type); beyond: the tile GEMM)
constexpr int FQ_MM_TILE_ROWS = 32;                        // weight rows of a tile of the tile GEMM (GQ_TM)
constexpr int FQ_MM_SK_TM = 32, FQ_MM_SK_TN = 16, FQ_MM_SK_GS = 32;      // streaming forms: rows per workgroup, columns per pass, blocks per stage (SK_TM, SK_TN, SK_GS)
constexpr int FQ_MM_KS_TMAX = 8;                           // tiles (consumer waves) per workgroup of the self-paced forms (KS_TMAX)
constexpr int FQ_MM_KQ_SEG = 32, FQ_MM_K2_SEG = 16;        // super-blocks per segment of the k-quant streaming forms (KQ_SEG: Q4_K / Q5_K; K2_SEG: Q2_K / Q3_K / Q6_K)
constexpr size_t FQ_MM_LDS_MAX = 160 * 1024;

// (Q4_K / Q5_K at model widths: up to five passes -- Falcon-40B, 12 blocks: 48 columns 6.0 against 10.4 ms, 64: 7.9 against 10.7, 80: 9.8 against ~11; 96: 11.7 against 11.3.
// Q2_K, 12 blocks of Falcon-40B: 80 columns 7.6 against ~11.6 ms, 128: 12.2 against 11.8)
static inline int fq_skinny_kq_max_cols(int type) { return (type == FQ_Q2_K || type == FQ_Q3_K) ? 112 : 80; }
static inline bool fq_mm_legacy(int t) { return t == FQ_Q4_0 || t == FQ_Q4_1 || t == FQ_Q5_0 || t == FQ_Q5_1 || t == FQ_Q8_0; }
static inline bool fq_mm_kquant(int t) { return t == FQ_Q2_K || t == FQ_Q3_K || t == FQ_Q4_K || t == FQ_Q5_K || t == FQ_Q6_K; }

// ---- the environment switches of the mat-mul dispatch and of launch_stage, each named once. All are latched at the process's first use (fq_mm_sw());
// FQ_GEMM_CFG alone is read per call (fq_mm_env_cfg()): the tests set it mid-process.
struct fq_mm_switches {
    bool    gemm_skinny   = true;      // FQ_GEMM_SKINNY=0: the tile GEMM for every N > 4 (no streaming, paired or fused form)
    bool    gemm_skinny2  = true;      // FQ_GEMM_SKINNY2=0: no passes of 16 beyond 16 columns
    bool    small_tt      = true;      // FQ_GEMM_SMALL_TT=0: 128-token tiles also at N <= 64
    bool    fill          = false;     // FQ_GEMM_FILL=1: 64-token workgroups where 128-token ones leave CUs empty (measured slower)
    bool    seq16         = true;      // FQ_GEMM_SEQ16=0: the sequential sum of the legacy formats through <1, 4> at every N
    int64_t rb_tiles      = -1;        // FQ_GEMM_RB_TILES=n: 64-row workgroups from n x #CU tiles on, at every length
    int64_t rb_tiles_long = 8;         // FQ_GEMM_RB_TILES_LONG=n: that threshold from 512 tokens on
    int64_t rb_tiles_mid  = 4;         // FQ_GEMM_RB_TILES_MID=n: .. at 256..511 tokens, legacy formats
    bool    rb_big_m      = true;      // FQ_GEMM_RB_BIG_M=0: no 64-row workgroups at 97..128 tokens for the matrices that fill the chip twice over
    bool    pair          = true;      // FQ_SKINNY_PAIR=0: Wqkv and Wup never in one launch
    bool    pair2         = true;      // FQ_SKINNY_PAIR2=0: .. not as two passes at 17..32 columns
    bool    ks            = true;      // FQ_SKINNY_KS=0: no K-share form (long rows: the plain streaming form)
    bool    out2          = true;      // FQ_SKINNY_OUT2=0: Wdown and Wo never in one K-share launch
    bool    res           = true;      // FQ_SKINNY_RES=0: no resident-column form
    bool    q4k           = true;      // FQ_SKINNY_Q4K=0: no streaming form of the k-quants
    bool    q4k_fused     = true;      // FQ_SKINNY_Q4K_FUSED=0: no fused sum launches (gelu + Q8_K, Wo + Wdown) of the k-quants
    bool    q4k_fused2    = true;      // FQ_SKINNY_Q4K_FUSED2=0: .. not in passes beyond 16 columns
    int64_t kqref_max_n   = INT64_MAX; // FQ_KQREF_MAX_N=n: reference order 2, k-quants: one thread per output beyond n columns
    bool    cols_max_set  = false;     // FALCON_HIP_COLS_MAX_N present at all: k-quant models at model widths keep the column kernels beyond 2 sequences
    int     cols_max_n    = 0;         // FALCON_HIP_COLS_MAX_N=n > 0: the column mat-vec kernels for lock-step contexts of up to n sequences
    bool    quant_rider   = true;      // FALCON_HIP_QUANT_RIDER=0: gelu(up)'s image by a launch of its own, never on the decode attention launch
    int     par2_min_n    = 0;         // FALCON_HIP_PAR2_MIN_N=n: the two-stream form from n rows (default 17 tokens / 33 sequences)
    bool    par2_seqs     = true;      // FALCON_HIP_PAR2_SEQS=0: lock-step passes always in stream order
    int     par2_down_first = 1;       // FALCON_HIP_PAR2_DOWN_FIRST=0: Wdown never ahead of the attention branch (the epilogue form), 2: always
};
static inline bool fq_mm_env_on(const char * name)  { const char * e = getenv(name); return !(e && atoi(e) == 0); }      // default on
static inline bool fq_mm_env_set(const char * name) { const char * e = getenv(name); return e && atoi(e) != 0; }         // default off
static inline int64_t fq_mm_env_i64(const char * name, int64_t dflt) { const char * e = getenv(name); return e ? atoll(e) : dflt; }
static inline fq_mm_switches fq_mm_switches_from_env() {
    fq_mm_switches s;
    s.gemm_skinny = fq_mm_env_on("FQ_GEMM_SKINNY");   s.gemm_skinny2 = fq_mm_env_on("FQ_GEMM_SKINNY2");
    s.small_tt = fq_mm_env_on("FQ_GEMM_SMALL_TT");    s.fill = fq_mm_env_set("FQ_GEMM_FILL");          s.seq16 = fq_mm_env_on("FQ_GEMM_SEQ16");
    s.rb_tiles = fq_mm_env_i64("FQ_GEMM_RB_TILES", -1); s.rb_tiles_long = fq_mm_env_i64("FQ_GEMM_RB_TILES_LONG", 8); s.rb_tiles_mid = fq_mm_env_i64("FQ_GEMM_RB_TILES_MID", 4);
    s.rb_big_m = fq_mm_env_on("FQ_GEMM_RB_BIG_M");
    s.pair = fq_mm_env_on("FQ_SKINNY_PAIR");          s.pair2 = fq_mm_env_on("FQ_SKINNY_PAIR2");       s.ks = fq_mm_env_on("FQ_SKINNY_KS");
    s.out2 = fq_mm_env_on("FQ_SKINNY_OUT2");          s.res = fq_mm_env_on("FQ_SKINNY_RES");           s.q4k = fq_mm_env_on("FQ_SKINNY_Q4K");
    s.q4k_fused = fq_mm_env_on("FQ_SKINNY_Q4K_FUSED"); s.q4k_fused2 = fq_mm_env_on("FQ_SKINNY_Q4K_FUSED2");
    s.kqref_max_n = fq_mm_env_i64("FQ_KQREF_MAX_N", INT64_MAX);
    s.cols_max_set = getenv("FALCON_HIP_COLS_MAX_N") != nullptr; s.cols_max_n = (int) fq_mm_env_i64("FALCON_HIP_COLS_MAX_N", 0);
    s.quant_rider = fq_mm_env_on("FALCON_HIP_QUANT_RIDER");
    s.par2_min_n = (int) fq_mm_env_i64("FALCON_HIP_PAR2_MIN_N", 0); s.par2_seqs = fq_mm_env_on("FALCON_HIP_PAR2_SEQS");
    s.par2_down_first = (int) fq_mm_env_i64("FALCON_HIP_PAR2_DOWN_FIRST", 1);
    return s;
}
inline const fq_mm_switches & fq_mm_sw() { static const fq_mm_switches s = fq_mm_switches_from_env(); return s; }
// FQ_GEMM_CFG=c, read per call: every tile GEMM launch as cfg c (0 = <1,4>, 1 = <4,1>, 2 = <4,4>, 3 = <2,4>, 4 = <4,2>, 5 = <2,2>, 6 = <2,4,2>, 7 = <4,4,2>), and no
// streaming, paired or fused form while it is set. -1: not set
static inline int fq_mm_env_cfg() { const char * e = getenv("FQ_GEMM_CFG"); return e ? atoi(e) : -1; }

// the process modes a decision depends on
struct fq_mm_mode {
    int  ref_order  = 0;               // ggml_hip_reference_order: 0 default, 1 one thread per output, 2 the same association on the fast kernels
    bool sequential = false;           // fq_gemm_set_sequential: every GEMM shape through S = 1 (set with ref_order != 0, or alone)
    bool force_gemv = false;           // ggml_hip_debug_force_gemv
    int  forced_cfg = -1;              // fq_mm_env_cfg()
};

// what the rules read of a weight matrix
struct fq_mm_mat { int type; int64_t M, form_M, K, nblk; size_t row_stride; };
static inline fq_mm_mat fq_mm_mat_of(const fq_weight & w) { return fq_mm_mat{ w.type, w.M, fq_form_rows(w), w.K, w.nblk, w.row_stride }; }
static inline fq_mm_mat fq_mm_mat_make(int type, int64_t M, int64_t K) {
    const fq_type_desc d = fq_desc(type);
    return fq_mm_mat{ type, M, M, K, d.blck ? K / d.blck : 0, d.blck ? fq_il_row_stride(d, K / d.blck) : (size_t) K * 2 };
}

enum fq_mm_family {
    FQ_MM_F16 = 0,        // kernels_f16.hip: one order for every N and mode
    FQ_MM_REF,            // kernels_ref.hip: one thread per output
    FQ_MM_KQREF,          // kernels_kqref.hip, column by column (where its LDS does not fit the launcher refuses: FQ_MM_REF)
    FQ_MM_GEMV,           // the column mat-vec in chunks of 4 / 2 / 1
    FQ_MM_STREAM,         // the streaming small-batch forms, passes of 16 columns
    FQ_MM_TILE,           // the int8-MFMA tile GEMM k_gemm_q<S, TT, RB>
};
enum fq_mm_stream_kind { FQ_MM_SK_NONE = 0, FQ_MM_SK_RES, FQ_MM_SK_KSHARE, FQ_MM_SK_PLAIN, FQ_MM_SK_KQ };
struct fq_mm_form {
    int family;
    int S;                // K split = the association of a row's sum (1, 2, 4); 0 where the family has one order only
    int cfg;              // FQ_MM_TILE: the tile cfg (16 = SEQ16), else -1
    int passes, pass_w;   // launches of the family and the columns of one (GEMV: the first chunk's width)
    int wg_rows, tile_cols;      // FQ_MM_TILE / FQ_MM_STREAM: weight rows per workgroup and the token-tile width
    int stream_kind;      // FQ_MM_STREAM: which of the streaming forms
    bool uses_scratch;    // writes the process-wide partial-sum scratch (hip_context::ks_scratch): the K-share form and the k-quants' streaming forms
};

// ---- LDS arithmetic of the legacy streaming forms (kernels_gemm_skinny.hip: sk_fmt / sk_res / ks_fmt; their launchers size the launch with these)
// bytes of a row's stage in LDS, padded to an ODD number of 16-byte slots (the 16 rows of a tile in distinct banks)
constexpr int fq_mm_sk_rowb(int type) {
    const fq_type_desc d = fq_desc(type);
    const int pb2 = d.nplanes > 2 ? d.plane[2].bytes : 0;
    const int rowd = FQ_MM_SK_GS * (d.plane[0].bytes + d.plane[1].bytes + pb2) + (pb2 ? 16 : 0);
    return ((rowd / 16) % 2 == 0) ? rowd + 16 : rowd;
}
// the resident form: the N columns in LDS for the whole launch (K up to ~4.6 k for Q4_0), nbw weight stages
static inline size_t fq_mm_res_lds(int type, int64_t nblk, int S, int nbw) {
    const int q = (int) nblk * 32, tqs = q + ((16 - (q & 255)) & 255);
    return (size_t) nbw * FQ_MM_SK_TM * fq_mm_sk_rowb(type) + (size_t) FQ_MM_SK_TN * tqs + 2 * (size_t) nblk * FQ_MM_SK_TN * 4 + (S > 1 ? 2 * (size_t)(S - 1) * 2 * 64 * 16 : 0);
}
static inline int fq_mm_res_nbw(int type, int64_t nblk, int S) {             // weight stages of the resident form: 3, 2, or 0 = the columns do not fit
    if (!fq_mm_legacy(type)) return 0;
    for (int n : { 3, 2 }) if (fq_mm_res_lds(type, nblk, S, n) <= FQ_MM_LDS_MAX) return n;
    return 0;
}
// the K-share form: one K share per workgroup, T 16-row tiles, a quarter of the columns' bytes resident
constexpr int fq_mm_ks_wstage(int type) {
    const fq_type_desc d = fq_desc(type);
    const int qb = d.plane[0].bytes, pb2 = d.nplanes > 2 ? d.plane[2].bytes : 0;
    const int np = 8 * (qb / 16) + 32 * d.plane[1].bytes / 16 + (pb2 ? 32 * pb2 / 16 + 1 : 0);
    return 16 * 16 * ((np % 2) ? np : np + 1);
}
static inline size_t fq_mm_ks_lds(int type, int64_t nblk, int T, int nbw) {
    const int q = (((int) nblk + 3) / 4) * 32, tqs = q + ((16 - (q & 255)) & 255);
    return (size_t) nbw * T * fq_mm_ks_wstage(type) + (size_t) FQ_MM_SK_TN * tqs + 2 * (size_t)(((int) nblk + 3) / 4) * FQ_MM_SK_TN * 4;
}
// its plan for a matrix: tiles per workgroup (all workgroups resident in one round, or full workgroups that walk their row blocks), row blocks, slots, grid
struct fq_mm_ks_plan { int T, nrb, nslots; unsigned grid; };
static inline fq_mm_ks_plan fq_mm_ks_make_plan(int64_t M, int n_cu) {
    const int ntiles = (int)((M + 15) / 16);
    int T = (ntiles * 4 + n_cu - 1) / n_cu;
    if (T < 1) T = 1;
    if (T > FQ_MM_KS_TMAX) T = FQ_MM_KS_TMAX;
    const int nrb = (ntiles + T - 1) / T;
    int nslots = 8 * ((nrb + 7) / 8);
    if (4 * nslots > n_cu) nslots = (n_cu / 32) * 8 > 8 ? (n_cu / 32) * 8 : 8;      // (never an empty grid on a part with fewer than 32 CUs)
    return fq_mm_ks_plan{ T, nrb, nslots, (unsigned)(4 * nslots) };
}
static inline int fq_mm_ks_nbw(int type, int64_t nblk, int T) {
    for (int n : { 3, 2 }) if (fq_mm_ks_lds(type, nblk, T, n) <= FQ_MM_LDS_MAX) return n;
    return 0;
}
// would fq_launch_gemm_skinny's K-share branch take this matrix (after the resident form refused it)? long rows whose columns do not fit: four partial sums per
// row in the process-wide scratch
static inline bool fq_mm_kshare_shape(const fq_mm_mat & w, int S, int n_cu, const fq_mm_switches & sw) {
    return sw.ks && fq_mm_legacy(w.type) && S == 4 && w.M <= FQ_KS_MAX_M && w.nblk >= 256 && fq_mm_ks_nbw(w.type, w.nblk, fq_mm_ks_make_plan(w.M, n_cu).T) != 0;
}

// Q4_K / Q5_K / Q2_K / Q3_K / Q6_K matrices the k-quants' streaming forms take (kernels_gemm_skinny_k.hip; the oracle's mode 2 follows the same rule).
// The decision from the rows of the whole matrix (a row-split part follows the matrix it is a part of; fq_weight_upload_part pads a part to whole 16-row tiles
// so that it can), the part's own rows only have to fit the form
static inline bool fq_mm_q4k_shape(const fq_mm_mat & w, const fq_mm_switches & sw) {
    const int seg = (w.type == FQ_Q2_K || w.type == FQ_Q3_K || w.type == FQ_Q6_K) ? FQ_MM_K2_SEG : FQ_MM_KQ_SEG;
    const int64_t Mf = w.form_M;
    const int64_t nseg = (w.nblk + seg - 1) / seg, mstride = (Mf + 63) & ~(int64_t) 63;
    return sw.q4k && fq_mm_kquant(w.type) && Mf % 16 == 0 && w.M % 16 == 0 && w.M <= Mf &&
           nseg * 4 * FQ_MM_SK_TN * mstride <= (int64_t) FQ_KS_FLOATS && w.nblk >= 8 && w.K < ((int64_t) 1 << 24) && w.row_stride * 16 < ((size_t) 1 << 31);
}

// ---- the k-quants' streaming forms (kernels_gemm_skinny_k.hip): a workgroup's LDS and the plan of a launch -- tiles (waves) per workgroup, weight stages, row
// blocks and the row-block slots of a K segment. The launchers run this plan; the kernels carve LDS up by their own kq_lds / k2_lds / k6_lds, whose totals the
// launchers hold against fq_mm_kq_lds.
static inline size_t fq_mm_kq_lds(int type, int seg_sb, int T, int nbw) {
    const bool q45 = type == FQ_Q4_K || type == FQ_Q5_K;
    const int rowp = (type == FQ_Q4_K || type == FQ_Q2_K) ? 21 : 29;                   // 16-byte slots per row and stage (kq_fmt / k2_fmt::ROWP, K6_ROWP)
    const int qb = seg_sb * (q45 ? 128 : 256), tqs = qb + ((16 - (qb & 255)) & 255);
    const size_t rings = (size_t) nbw * T * 16 * 16 * rowp, cols = (size_t) FQ_MM_SK_TN * tqs, dy = (size_t) seg_sb * FQ_MM_SK_TN * 4;
    if (q45) return rings + cols + dy + (size_t) seg_sb * FQ_MM_SK_TN * 16 + 16;
    if (type == FQ_Q6_K) return rings + cols + dy;
    return rings + cols + dy + (type == FQ_Q3_K ? 0 : (size_t) seg_sb * FQ_MM_SK_TN * 32) + 32;
}
struct fq_mm_kq_plan { int nseg, seg_sb, T, nbw, nrb, nslots; size_t lds; };            // nbw 0: no carve-up fits, the form refuses
// M rows (whole 16-row tiles), nblk super-blocks per row. env_t / env_nbw: the tuning aids FQ_KQ_T / FQ_KQ_NBW (0: not set)
static inline fq_mm_kq_plan fq_mm_kq_make_plan(int type, int64_t M, int64_t nblk, int n_cu, int env_t = 0, int env_nbw = 0) {
    const bool q45 = type == FQ_Q4_K || type == FQ_Q5_K;
    const bool three = type == FQ_Q4_K || type == FQ_Q2_K;                             // (Q5_K, Q3_K: 8 DMA instructions per stage -- two stages ahead would pass vmcnt's 15; Q6_K: two stages)
    const int seg = q45 ? FQ_MM_KQ_SEG : FQ_MM_K2_SEG, ntiles = (int)(M / 16), nsb = (int) nblk;
    fq_mm_kq_plan p{};
    p.nseg = (nsb + seg - 1) / seg;
    p.seg_sb = p.nseg > 1 ? seg : (q45 ? ((nsb + 7) & ~7) : ((nsb + 3) & ~3));         // (LDS is sized by it; stages of 4 super-blocks never straddle a column of the device layout)
    p.T = env_t > 0 ? env_t : (ntiles * (q45 ? 2 : 1) * p.nseg + n_cu - 1) / n_cu;     // tiles per workgroup: all workgroups resident in one round when they fit
    if (p.T < 1) p.T = 1;
    if (p.T > FQ_MM_KS_TMAX) p.T = FQ_MM_KS_TMAX;
    for (;;) {
        for (int n : { 3, 2 }) {
            if ((env_nbw && n != env_nbw) || (n == 3 && !three)) continue;
            if (fq_mm_kq_lds(type, p.seg_sb, p.T, n) <= FQ_MM_LDS_MAX) { p.nbw = n; break; }
        }
        if (p.nbw || p.T == 1) break;
        --p.T;
    }
    if (!p.nbw) return p;
    p.lds = fq_mm_kq_lds(type, p.seg_sb, p.T, p.nbw);
    p.nrb = (ntiles + p.T - 1) / p.T;
    if (q45) {                                                                         // a pair of workgroups (shares {0, 1} and {2, 3}) per (row block, segment), slots in eights (one XCD)
        p.nslots = 8 * ((p.nrb + 7) / 8);
        const int cap = ((n_cu / (2 * p.nseg)) / 8) * 8;                               // row-block slots per segment when the launch is larger than the chip
        if (2 * p.nslots * p.nseg > n_cu) p.nslots = cap < 8 ? 8 : (p.nslots < cap ? p.nslots : cap);
    } else {                                                                           // more (row block, segment) pairs than CUs: persistent workgroups in full rounds, unless the last round would be nearly empty
        p.nslots = p.nrb;
        if (p.nrb * p.nseg > n_cu) { const int cap = n_cu / p.nseg > 0 ? n_cu / p.nseg : 1; if (p.nrb % cap == 0 || p.nrb > 2 * cap) p.nslots = cap; }
    }
    return p;
}

// ---- the tile GEMM
// The unit of parallelism is a 32-token x 32-row tile (568 of them for a 4544-row matrix and 128 tokens), split S ways
// over K. Measured on MI355X, Falcon-7B shapes, Q4_0 (scripts/gpu_gemm_prof.sh), us for qkv / wo / up / down:
//   128 tokens   <S 1, 4 tiles>  44 / 44 /  92 / 163    <S 2, 4 tiles>  34 / 34 /  82 / 119    <S 4, 4 tiles>  31 / 31 /  95 / 106
//   512 tokens   <S 1, 4 tiles>  94 / 93 / 265 / 340    <S 2, 4 tiles>  83 / 83 / 242 / 296    <S 4, 4 tiles>  94 / 94 / 290 / 331
//   2048 tokens  <S 1, 4 tiles> 287 / 266 / 1043 / 1038 <S 2, 4 tiles> 259 / 238 / 969 / 929   <S 4, 4 tiles> 316 / 289 / 1157 / 1061
// -> four partial sums per row below 4 x #CU tiles, two above; one (the reference's order) only on request
static inline int64_t fq_mm_tiles(int64_t form_rows, int64_t N) { return ((form_rows + FQ_MM_TILE_ROWS - 1) / FQ_MM_TILE_ROWS) * ((N + 31) / 32); }   // (a row-split part: the whole matrix's tiles, fq_types.h)
// the K split (1, 2, 4) an M x N result gets: the same in the tile GEMM and in every streaming form ("same K split -> same bits")
static inline int fq_mm_split(int64_t form_rows, int64_t N, int n_cu, bool sequential) {
    if (sequential) return 1;
    return fq_mm_tiles(form_rows, N) < 4 * (int64_t) n_cu ? 4 : 2;
}
// the 64-row workgroups' threshold (x #CU tiles of 32 x 32; 0 = never) by prompt length
static inline int64_t fq_mm_rb_min(int64_t N, int type, int64_t M, int n_cu, const fq_mm_switches & sw) {
    // (256 tokens included: a prompt of 256 does not move, 12.0 ms, a lock-step pass of 256 sequences does, 14.76 -> 13.18 ms, profiles/r06zzf_lockstep_sweep.txt)
    // (the 256..511 rule for the legacy formats only: the k-quants' integer-domain GEMM loses with 64-row workgroups there -- Falcon-40B Q2_K 288-384 tokens 29-30 -> 32.5-33 ms,
    // Q4_K 23.0-23.8 -> 23.8-24.4; profiles/r06zzd_ab_rb_mid.txt)
    // (Q4_K / Q5_K below 512 tokens: 8 x #CU except at three token tile rows -- Falcon-40B shapes, 12 blocks, threshold 32 -> 8: Q4_K 128 tokens 8.91 -> 8.42 ms, 256: 16.24 -> 14.92,
    // 448: 31.06 -> 28.65, lock-step 128 / 256 per pass 9.34 -> 9.00 / 18.14 -> 17.03, but 320-384 tokens 23.4-24.0 -> 23.9-24.4; Q5_K alike; Q2_K loses up to 11 % with it and keeps 32
    // (profiles/r06zzi_kq_rb.txt, r06zzj_kq_rb8.txt))
    if (sw.rb_tiles >= 0) return sw.rb_tiles;
    if (N >= 512) return sw.rb_tiles_long;
    if (type == FQ_Q4_K || type == FQ_Q5_K) return (N + 127) / 128 == 3 ? 32 : 8;
    // (one token tile row, legacy formats: only a matrix whose 64-row workgroups still fill the chip twice over -- Falcon-40B's Wup: 512 of them; 128-token prompt 8.65 -> 8.23 ms on
    // Falcon-40B Q5_1 shapes, profiles/r06zzl_*, r06zzm_*; Falcon-7B's 284 lose: 6.8 -> 7.27 ms; a full tile row only: at 40-96 tokens the same matrix loses 2-5 % as a prompt
    // and wins 12 % as a lock-step pass of 64 -- left alone)
    if (sw.rb_big_m && N > 96 && N <= 128 && fq_desc(type).blck == 32 && (M + 63) / 64 >= 2 * (int64_t) n_cu) return 1;
    return N >= 256 && fq_desc(type).blck == 32 ? sw.rb_tiles_mid : 32;
}
// K split, weight rows per workgroup and token-tile width of a tile cfg: k_gemm_q<S, TT, RB> = 32 RB rows x 32 TT tokens
static inline int fq_mm_cfg_split(int cfg)     { return (cfg == 0 || cfg == 16) ? 1 : ((cfg == 3 || cfg == 5 || cfg == 6) ? 2 : 4); }
static inline int fq_mm_cfg_wg_rows(int cfg)   { return (cfg >= 0 && cfg <= 5) || cfg == 16 ? 32 : 64; }      // (any other value launches <4,4,2>, as cfg 7)
static inline int fq_mm_cfg_tile_cols(int cfg) { return cfg == 1 ? 32 : ((cfg == 4 || cfg == 5) ? 64 : 128); }
// the cfg fq_launch_gemm's tile form gives an M-row matrix at N columns
static inline int fq_mm_tile_cfg(int type, int64_t form_rows, int64_t N, int n_cu, const fq_mm_mode & md, const fq_mm_switches & sw) {
    const int64_t tiles = fq_mm_tiles(form_rows, N);
    int cfg = md.sequential ? 0 : (tiles < 4 * (int64_t) n_cu ? 2 : 3);
    // 64-row workgroups (RB = 2) where there are tiles enough to fill the chip with them: two partial sums as <2,4> above,
    // or four (<4,4,2>: 16 waves) for the formats whose 64-row kernel stays within 128 VGPRs
    // (round 6: from 512 tokens on already at 8 x #CU tiles -- the short matrices of a long prompt (Wqkv, Wo, Wdown: 4 672 tiles at 1024 tokens) had fallen between the two
    // rules: Falcon-7B Q4_0 1024 tokens 40.7 -> 36.8 ms, 512: 22.75 -> 22.27; below 512 tokens the same threshold costs Wup 6 % at 256 and 7 % at 128. The same S: the same bits.
    // FQ_GEMM_RB_TILES=n: n x #CU for every length (A/B, profiles/r06zz_ab_rb_tiles.txt); FQ_GEMM_RB_TILES_LONG=n: the threshold from 512 tokens on)
    // (and from 257 tokens on at 4 x #CU -- every matrix of a block that takes two partial sums: three token tile rows were the other hole, 288-384 tokens 16.4-17.6 -> 13.8-14.6 ms
    // together with the residual-sum launch of falcon_stage.hip, profiles/r06zzc_*; FQ_GEMM_RB_TILES_MID=n)
    { const int64_t rbm = fq_mm_rb_min(N, type, form_rows, n_cu, sw); if (cfg == 3 && rbm > 0 && tiles >= rbm * (int64_t) n_cu) cfg = 6; }
    // few columns (round 6): token tiles of 32 / 64 instead of 128 -- the same four-way K split (S = 4: the same association, the same bits), a quarter /
    // half of the matrix work on padding columns gone and 4 / 8 waves per workgroup instead of 16 (FQ_GEMM_SMALL_TT=0: the 128-token tiles, as before)
    if (sw.small_tt && cfg == 2 && N <= 32) cfg = 1; else if (sw.small_tt && cfg == 2 && N <= 64) cfg = 4;
    // (tuning aid, FQ_GEMM_FILL=1: a launch of 128-token workgroups that leaves CUs empty -- 142 workgroups for a 4544-row matrix and 128 tokens -- as 64-token
    // workgroups, 284 of them: measured SLOWER, 128-token prompt 9.46 against 8.30-8.34 ms A/B/A/B on one box (round 6): the 16-wave workgroup hides its own latencies better
    // than two 8-wave ones fill the chip)
    if (sw.fill && cfg == 2 && N > 64 && ((form_rows + FQ_MM_TILE_ROWS - 1) / FQ_MM_TILE_ROWS) * ((N + 127) / 128) < n_cu) cfg = 4;
    if (md.forced_cfg >= 0) cfg = md.forced_cfg;                                // tuning override (fq_mm_env_cfg)
    // the sequential sum of the legacy formats: sixteen 16 x 16 tiles per workgroup instead of four 32 x 32 ones (SEQ16, k_gemm_q's header; FQ_GEMM_SEQ16=0: the S = 1 form)
    // one tile row of tokens only: measured on MI355X, Falcon-7B Q4_0 prompts in the fast reference order, SEQ16 against S = 1 (scripts/gpu_prompt_lengths.py, A/B/A/B):
    // 40 tokens 10.3 against 12.2 ms, 64: 10.5 / 12.6, 128: 11.7 / 13.3 -- but 256: 21.4 / 18.1, 512: 39.4 / 31.9, 2048: 194 / 171-180: with several token tile rows the S = 1
    // form has the waves to fill its chains and the 16 x 16 tiles' extra operand reads cost more than they hide
    if (cfg == 0 && sw.seq16 && fq_desc(type).blck == 32 && N <= 128) cfg = 16;
    return cfg;
}

// ---- fq_launch_gemm: one matrix at N columns (the caller has decided for the GEMM side: N > 4, or the cases of fq_mm_form_of below)
// small batches: the streaming form (kernels_gemm_skinny.hip), same K split -> same bits (FQ_GEMM_SKINNY=0: the tile GEMM for every N).
// 17..32 columns: two passes of the streaming form (same K split as this shape's tile GEMM, so the same bits; 7.5 against 9.1 ms
// per Falcon-7B pass of 32 lock-step sequences) -- beyond that the tiles win. The k-quants at model widths: up to fq_skinny_kq_max_cols columns
static inline int64_t fq_mm_stream_max_cols(const fq_mm_mat & w, const fq_mm_mode & md, const fq_mm_switches & sw) {
    if (!sw.gemm_skinny || md.forced_cfg >= 0) return 0;
    if (!sw.gemm_skinny2) return 16;
    return fq_mm_q4k_shape(w, sw) ? fq_skinny_kq_max_cols(w.type) : 32;
}
// which streaming form takes one pass of <= 16 columns at K split S (FQ_MM_SK_NONE: none does, fq_launch_gemm_skinny refuses)
static inline int fq_mm_stream_kind_of(const fq_mm_mat & w, int S, int n_cu, const fq_mm_switches & sw) {
    if (fq_mm_kquant(w.type)) return S != 1 && fq_mm_q4k_shape(w, sw) ? FQ_MM_SK_KQ : FQ_MM_SK_NONE;
    if (!fq_mm_legacy(w.type)) return FQ_MM_SK_NONE;
    if (sw.res && fq_mm_res_nbw(w.type, w.nblk, S)) return FQ_MM_SK_RES;      // the columns resident in LDS, one persistent workgroup per CU, when they fit
    if (fq_mm_kshare_shape(w, S, n_cu, sw)) return FQ_MM_SK_KSHARE;            // long rows (the columns do not fit): one K share per workgroup
    return FQ_MM_SK_PLAIN;
}
static inline fq_mm_form fq_mm_gemm_form(const fq_mm_mat & w, int64_t N, int n_cu, const fq_mm_mode & md, const fq_mm_switches & sw) {
    fq_mm_form f{ FQ_MM_TILE, 0, -1, 1, (int) N, 0, 0, FQ_MM_SK_NONE, false };
    const int S = fq_mm_split(w.form_M, N, n_cu, md.sequential);
    if (N <= fq_mm_stream_max_cols(w, md, sw)) {
        const int kind = fq_mm_stream_kind_of(w, S, n_cu, sw);
        if (kind != FQ_MM_SK_NONE) {
            f.family = FQ_MM_STREAM; f.S = S; f.passes = (int)((N + 15) / 16); f.pass_w = N < 16 ? (int) N : 16;
            f.wg_rows = FQ_MM_SK_TM; f.tile_cols = FQ_MM_SK_TN; f.stream_kind = kind;
            f.uses_scratch = kind == FQ_MM_SK_KSHARE || kind == FQ_MM_SK_KQ;
            return f;
        }
    }
    f.cfg = fq_mm_tile_cfg(w.type, w.form_M, N, n_cu, md, sw);
    f.S = fq_mm_cfg_split(f.cfg); f.wg_rows = fq_mm_cfg_wg_rows(f.cfg); f.tile_cols = fq_mm_cfg_tile_cols(f.cfg);
    return f;
}

// ---- the fused sum launches of the k-quants' streaming forms (gelu + Q8_K image, Wo + Wdown): 5..16 columns (lock-step contexts: from min_cols = 3), default order
static inline bool fq_mm_q4k_fused_ok(int64_t N, int64_t min_cols, const fq_mm_mode & md, const fq_mm_switches & sw) {
    return sw.gemm_skinny && md.forced_cfg < 0 && sw.q4k_fused && !md.ref_order && !md.force_gemv && !md.sequential && N >= min_cols && N <= 16;
}
// (round 6) 17 .. fq_skinny_kq_max_cols columns -- the widths fq_launch_gemm runs as passes of 16 of the same form -- keep the fused sum launches: one pass of 16 columns at a time
static inline bool fq_mm_q4k_fused_passes(const fq_mm_mat & w, int64_t N, const fq_mm_mode & md, const fq_mm_switches & sw) {
    return sw.gemm_skinny2 && sw.q4k_fused2 && N > 16 && fq_mm_q4k_shape(w, sw) && N <= fq_skinny_kq_max_cols(w.type) && fq_mm_q4k_fused_ok(16, FQ_GEMV_MAX_COLS + 1, md, sw);
}

// ---- fq_mul_mat_q_acts: one matrix at N columns, every family. from3 (fq_mul_mat_q_acts_from3): lock-step contexts of 3 and 4 sequences on the k-quant formats
// with a streaming form at this shape take it (a pass of 16 columns costs less than the column mat-vec kernels' pass of 4 there: Falcon-40B Q2_K 8.2 against
// 18.5 ms, Q4_K 9.9 against 15.2)
enum fq_mm_route { FQ_MM_TO_F16, FQ_MM_TO_REF, FQ_MM_TO_KQREF, FQ_MM_TO_GEMV, FQ_MM_TO_GEMM };      // which launcher: .. fq_launch_gemm (fq_mm_gemm_form says which of its forms)
static inline int fq_mm_route_of(const fq_mm_mat & w, int64_t N, const fq_mm_mode & md, const fq_mm_switches & sw, bool from3 = false) {
    if (w.type == FQ_F16) return FQ_MM_TO_F16;
    const bool gemm_type = fq_mm_legacy(w.type) || fq_mm_kquant(w.type);
    if (from3 && N >= 3 && N <= FQ_GEMV_MAX_COLS && fq_mm_q4k_fused_ok(N, 3, md, sw) && fq_mm_q4k_shape(w, sw)) return FQ_MM_TO_GEMM;
    // reference order: one thread per output (mode 1), or -- mode 2, legacy formats, batches -- the GEMM with S = 1 (one left-to-right sum per row, the scalar
    // build's two roundings per term: == the reference, tests/test_gpu_mul_mat.py)
    // (mode 2, legacy formats: from TWO columns on -- a lock-step context of 2-4 sequences is a 128-token tile of padding, still far ahead of one thread per output)
    if (md.ref_order && !(md.ref_order == 2 && fq_mm_legacy(w.type) && N >= 2 && !md.force_gemv)) {
        // mode 2, the k-quants: the wave-speed mat-vec in the reference's association (kernels_kqref.hip), column by column. A prompt re-reads the matrix per
        // token (out of L2 / the Infinity Cache) and is still 4.5 x faster than mode 1's one thread per output (Falcon-40B Q4_K, 128 tokens, 16 blocks: 268 against
        // 1 217 ms). FQ_KQREF_MAX_N=n: mode 1's kernel beyond n columns (A/B)
        // (and the legacy formats' single columns: the op-level API and the ggml-cuda.h shim; batches took the GEMM)
        return md.ref_order == 2 && N <= sw.kqref_max_n ? FQ_MM_TO_KQREF : FQ_MM_TO_REF;
    }
    if ((N > FQ_GEMV_MAX_COLS || (md.ref_order == 2 && N >= 2)) && gemm_type && !md.force_gemv) return FQ_MM_TO_GEMM;      // prefill: int8 MFMA GEMM
    return FQ_MM_TO_GEMV;
}
static inline fq_mm_form fq_mm_form_of(const fq_mm_mat & w, int64_t N, int n_cu, const fq_mm_mode & md, const fq_mm_switches & sw, bool from3 = false) {
    fq_mm_form f{ FQ_MM_F16, 0, -1, 1, (int) N, 0, 0, FQ_MM_SK_NONE, false };
    switch (fq_mm_route_of(w, N, md, sw, from3)) {
        case FQ_MM_TO_F16:   return f;
        case FQ_MM_TO_REF:   f.family = FQ_MM_REF; f.S = 1; return f;
        case FQ_MM_TO_KQREF: f.family = FQ_MM_KQREF; f.S = 1; f.passes = (int) N; f.pass_w = 1; return f;
        case FQ_MM_TO_GEMM:  return fq_mm_gemm_form(w, N, n_cu, md, sw);
        default: break;
    }
    f.family = FQ_MM_GEMV; f.pass_w = N >= 4 ? 4 : (N >= 2 ? 2 : 1);                  // chunks of 4, then 2, then 1
    f.passes = (int)(N / 4) + ((N & 2) ? 1 : 0) + (int)(N & 1);
    return f;
}

// ---- the launch key: the structural facts of the launch fq_mm_form_of plans -- which kernel instantiation runs and which of its code paths a workgroup takes --
// as integers, from the plan functions the launchers call. Two shapes with the same key (and format) run the same code; tests/test_mm_coverage_cpu.py holds
// the keys of the model matrices against those of the shapes the GPU tests run, ggml_hip_debug_mul_mat_plan returns the key of the device at hand.
//   [0] family  [1] S  [2] more than one pass  [3] stream kind, then by form:
//   TILE          [4] cfg  [5] more than one token-tile row  [6] ragged last row tile  [7] ragged last column tile
//   STREAM RES    [4] NBW  [5] workgroups loop (row pairs > #CU)  [6] ragged last 32-row pair
//   STREAM KSHARE [4] NBW  [5] T: 1 = one tile, 2 = 2..7, 3 = FQ_MM_KS_TMAX  [6] walk (row blocks > slots)  [7] ragged last 16-row tile
//   STREAM PLAIN  [6] ragged last 32-row tile
//   STREAM KQ     [4] kernel: 1 = q4k (Q4_K, Q5_K), 2 = q2k (Q2_K, Q3_K), 3 = q6k  [5] several K segments  [6] row blocks > slots (workgroups walk)  [7] NBW
constexpr int FQ_MM_KEY_LEN = 8;
static inline void fq_mm_launch_key(const fq_mm_mat & w, int64_t N, int n_cu, const fq_mm_mode & md, const fq_mm_switches & sw, bool from3, int * key) {
    const fq_mm_form f = fq_mm_form_of(w, N, n_cu, md, sw, from3);
    for (int i = 0; i < FQ_MM_KEY_LEN; ++i) key[i] = 0;
    key[0] = f.family; key[1] = f.S; key[2] = f.passes > 1; key[3] = f.stream_kind;
    if (f.family == FQ_MM_TILE) {
        key[4] = f.cfg; key[5] = N > f.tile_cols; key[6] = w.M % f.wg_rows != 0; key[7] = N % f.tile_cols != 0;
    } else if (f.family == FQ_MM_STREAM && f.stream_kind == FQ_MM_SK_RES) {
        key[4] = fq_mm_res_nbw(w.type, w.nblk, f.S); key[5] = (w.M + FQ_MM_SK_TM - 1) / FQ_MM_SK_TM > n_cu; key[6] = w.M % FQ_MM_SK_TM != 0;
    } else if (f.family == FQ_MM_STREAM && f.stream_kind == FQ_MM_SK_KSHARE) {
        const fq_mm_ks_plan pl = fq_mm_ks_make_plan(w.M, n_cu);
        key[4] = fq_mm_ks_nbw(w.type, w.nblk, pl.T); key[5] = pl.T == 1 ? 1 : (pl.T < FQ_MM_KS_TMAX ? 2 : 3); key[6] = pl.nrb > pl.nslots; key[7] = w.M % 16 != 0;
    } else if (f.family == FQ_MM_STREAM && f.stream_kind == FQ_MM_SK_PLAIN) {
        key[6] = w.M % FQ_MM_SK_TM != 0;
    } else if (f.family == FQ_MM_STREAM && f.stream_kind == FQ_MM_SK_KQ) {
        const bool k2 = w.type == FQ_Q2_K || w.type == FQ_Q3_K;
        key[4] = k2 ? 2 : (w.type == FQ_Q6_K ? 3 : 1);
        const fq_mm_kq_plan pl = fq_mm_kq_make_plan(w.type, w.M, w.nblk, n_cu);
        key[5] = pl.nseg > 1; key[6] = pl.nrb > pl.nslots; key[7] = pl.nbw;
    }
}

// ---- two matrices behind the same activation columns (Wqkv and Wup of a one-norm block) as ONE launch of the resident form: 5..16 columns, default order, same
// format / K / K split. (round 6) 17..32 columns: two passes of the pair launch, as fq_launch_gemm runs a single matrix of that width as two passes of the
// streaming form -- the same K split (one token tile row: the split does not change between 16 and 32 columns), the same bits, half the launches and the fuller
// grid of the pair. Returns the K split, 0: not eligible
static inline int fq_mm_pair_split(const fq_mm_mat & w0, const fq_mm_mat & w1, int act_type, int64_t act_K, int64_t N, int n_cu, const fq_mm_mode & md, const fq_mm_switches & sw) {
    if (!sw.gemm_skinny || md.forced_cfg >= 0 || !sw.pair || md.ref_order || md.force_gemv) return 0;
    if (N <= FQ_GEMV_MAX_COLS || N > (sw.pair2 && sw.gemm_skinny2 ? 32 : 16)) return 0;
    if (fq_desc(w0.type).act_type != act_type || act_K != w0.K || w1.K != w0.K || w1.type != w0.type || w0.nblk != w1.nblk) return 0;
    const int S0 = fq_mm_split(w0.M, N, n_cu, md.sequential), S1 = fq_mm_split(w1.M, N, n_cu, md.sequential);
    if (S0 != S1) return 0;
    if (N > 16 && (fq_mm_q4k_shape(w0, sw) || fq_mm_q4k_shape(w1, sw))) return 0;      // (the k-quants' streaming forms have their own passes)
    return sw.res && fq_mm_res_nbw(w0.type, w0.nblk, S0) ? S0 : 0;                   // (the pair launch is the resident form's)
}
// ---- x = (Wdown a_ff + Wo a_att) + x for the legacy formats: both matrices in the K-share form in ONE launch (k_gemm_skinny_ks2) and one sum launch;
// 17..32 columns as two passes of it (the streaming forms' own rule for that width)
struct fq_mm_out2_plan { bool ok; fq_mm_ks_plan down, wo; int nbw; size_t lds; };
static inline fq_mm_out2_plan fq_mm_out2_pass(const fq_mm_mat & wo, const fq_mm_mat & down, int att_type, int ff_type, int n_cu, const fq_mm_switches & sw) {      // one pass of <= 16 columns: fq_launch_gemm_skinny_out2
    fq_mm_out2_plan p{ false, {}, {}, 0, 0 };
    if (!sw.out2 || !sw.ks || wo.type != down.type || wo.M != down.M || wo.M > FQ_KS_MAX_M || !fq_mm_legacy(wo.type)) return p;
    if (down.nblk < 256 || wo.nblk < 32 || att_type != ff_type) return p;      // (Wdown alone would not take this form: leave the pair to the generic path)
    if ((size_t) 8 * FQ_MM_SK_TN * FQ_KS_MAX_M > (size_t) FQ_KS_FLOATS) return p;
    p.down = fq_mm_ks_make_plan(down.M, n_cu); p.wo = fq_mm_ks_make_plan(wo.M, n_cu);
    for (int n : { 3, 2 }) {
        const size_t nd = fq_mm_ks_lds(wo.type, down.nblk, p.down.T, n), nw = fq_mm_ks_lds(wo.type, wo.nblk, p.wo.T, n);
        p.lds = nd > nw ? nd : nw;
        if (p.lds <= FQ_MM_LDS_MAX) { p.nbw = n; break; }
    }
    p.ok = p.nbw != 0;
    return p;
}
static inline bool fq_mm_out2_legacy_ok(const fq_mm_mat & wo, const fq_mm_mat & down, int att_type, int ff_type, int64_t N, int n_cu, const fq_mm_mode & md, const fq_mm_switches & sw) {
    if (!sw.gemm_skinny || md.forced_cfg >= 0 || md.ref_order || md.force_gemv || N <= FQ_GEMV_MAX_COLS || N > (sw.gemm_skinny2 ? 32 : 16)) return false;
    if (fq_desc(wo.type).act_type != att_type || fq_desc(down.type).act_type != ff_type) return false;
    if (fq_mm_split(wo.M, N, n_cu, md.sequential) != 4 || fq_mm_split(down.M, N, n_cu, md.sequential) != 4) return false;
    return fq_mm_out2_pass(wo, down, att_type, ff_type, n_cu, sw).ok;
}

// ---- launch_stage's own rules
// lock-step contexts (and draft-and-verify passes) of up to this many rows run the column mat-vec kernels in chunks of 4 (FALCON_HIP_COLS_MAX_N overrides): 4 for the
// legacy formats, whose streaming small-batch mat-mul serves 5..16 columns in less time than two chunks (Falcon-7B Q4_0: 2.9 ms per pass
// against 3.6 at 8 sequences), 12 for k-quant models whose matrices are not at model widths (they have only the tile GEMM beyond).
// k-quant models at model widths (fq_mm_q4k_shape) have their own streaming forms and use them from 3 sequences up: a
// pass of 16 columns costs less there than the column kernels' pass of 4; contexts of 2 keep the column kernels and their bit-identity with a single stream.
// qkv0: Wqkv of the model's first block
static inline int fq_mm_cols_max_n(const fq_mm_mat & qkv0, const fq_mm_switches & sw) {
    if (fq_mm_q4k_shape(qkv0, sw) && !sw.cols_max_set) return 2;
    if (sw.cols_max_n > 0) return sw.cols_max_n;
    return fq_mm_legacy(qkv0.type) ? 4 : 12;
}
// The two-stream form runs {Wqkv, attention, Wo} on the main stream and {Wup, Wdown} on the side stream. The streaming forms that keep partial sums in the ONE
// process-wide scratch (the k-quants' passes, the legacy K-share form) must not run on both at once: a block in which a matrix of each branch would write the
// scratch at this N runs in stream order. (The k-quant passes fill the chip by themselves: any one of them keeps the block in stream order.)
static inline bool fq_mm_par2_scratch_clash(const fq_mm_mat & qkv, const fq_mm_mat & wo, const fq_mm_mat & up, const fq_mm_mat & down, int64_t N, int n_cu,
                                            const fq_mm_mode & md, const fq_mm_switches & sw) {
    auto kq_passes = [&](const fq_mm_mat & w) { return N <= fq_skinny_kq_max_cols(w.type) && fq_mm_q4k_shape(w, sw); };      // per matrix: a block may mix k-quant formats with different column limits
    if (kq_passes(qkv) || kq_passes(up) || kq_passes(wo) || kq_passes(down)) return true;
    auto scratch = [&](const fq_mm_mat & w) { return w.type != FQ_F16 && fq_mm_form_of(w, N, n_cu, md, sw).uses_scratch; };
    return (scratch(qkv) || scratch(wo)) && (scratch(up) || scratch(down));
}
// workgroups of one launch of a GEMM-side form (a streaming form's passes run one after the other: one pass). The two-stream form sends Wdown's launch first on
// the side stream when it is at most 1.25 rounds of the chip or at least 2
static inline int64_t fq_mm_gemm_wgs(const fq_mm_mat & w, int64_t N, int n_cu, const fq_mm_mode & md, const fq_mm_switches & sw) {
    const fq_mm_form f = fq_mm_gemm_form(w, N, n_cu, md, sw);
    return ((w.M + f.wg_rows - 1) / f.wg_rows) * (f.family == FQ_MM_STREAM ? 1 : (N + f.tile_cols - 1) / f.tile_cols);
}
