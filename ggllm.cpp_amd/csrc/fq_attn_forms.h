// fq_attn_forms.h -- which kernel a prompt (prefill) attention launch takes, and with what grid, LDS and scratch: ONE statement of the rules, as pure functions
// of the shape (N tokens, H / HKV heads, the launch's largest n_kv), the process modes, the environment switches, the chip's CUs and the scratch the caller can hand
// over. No HIP in here: g++ compiles it for tests/host/attn_forms_harness.cpp (tests/test_attn_forms_cpu.py pins the table). fq_launch_attention (kernels_attn.hip)
// launches from fq_attn_plan_of; a context's scratch is sized by fq_attn_scratch_need; the verify pair takes its LDS bytes from fq_attn_one_row_lds.
// The measured numbers behind every threshold stand next to the rule they justify. (The decode attention's FQ_ATTN_OUT_* switches live in kernels_decode.hip.)
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#ifndef FQ_ATTN_PACK_V
#define FQ_ATTN_PACK_V 1                                   // k_attn_pack_k also re-lays the values in pass C's operand order behind the keys
#endif

// ---- the environment switches of the prompt attention, each named once; latched at the process's first use (fq_attn_sw())
struct fq_attn_switches {
    int  rows         = -1;        // FQ_ATTN_ROWS=0,2,4,8: tokens per workgroup of k_attention_rows (0: k_attention, one token); set at all: never the matrix pipe
    bool mfma         = true;      // FQ_ATTN_MFMA=0: batches of 32 tokens and more through the rows forms instead of the f32 matrix pipe
    bool mfma16       = false;     // FQ_ATTN_MFMA16=1: form 16 (k_attention_mfma16: 16-token tiles, f32 scores in LDS) where no form is set
    bool mfma16h      = false;     // FQ_ATTN_MFMA16H=1: form 17 (k_attention_mfma16h: 16-token tiles, fp16 probabilities in LDS); wins over FQ_ATTN_MFMA16
    int  mfma16_maxkv = 4096;      // FQ_ATTN_MFMA16_MAXKV=n: form 16 up to n keys
    bool flash        = true;      // FQ_ATTN_FLASH=0: form 0 is the scratch form (k_attention_mfma), as before k_attention_flash
    bool flash_long   = true;      // FQ_ATTN_FLASH_LONG=0: beyond 74 key tiles the scratch form instead of k_attention_flash's LONG form
    bool flash_tab    = true;      // FQ_ATTN_FLASH_TAB=0: k_attention_flash computes exp() by the in-kernel formula where the caller passes no table
    bool keep         = true;      // FQ_ATTN_KEEP=0: k_attention_flash runs K.Q twice instead of keeping a wave's score tiles in registers
    bool persist      = true;      // FQ_ATTN_PERSIST=0: one workgroup per (head, query tile) instead of one per CU taking items from a counter
    int  pack_min_n   = 256;       // FQ_ATTN_PACK_MIN_N=n: the keys / values re-laid in operand order (k_attn_pack_k) from n tokens on
    bool scratch      = true;      // FQ_ATTN_SCRATCH=0: never 4 tokens per workgroup with the score rows in the global scratch
    int  scratch_gb   = 4;         // FQ_ATTN_SCRATCH_GB=n: no scratch beyond n GiB (the op-level API's process-wide buffer; the cap of a context's own)
    int  dbg          = 0;         // FQ_ATTN_DBG: bits 1 / 2 / 4 make k_attention_flash run pass A / B / C over no tiles (timing aid: results are garbage)
};
static inline int fq_attn_env_int(const char * name, int dflt) { const char * e = getenv(name); return e ? atoi(e) : dflt; }
static inline fq_attn_switches fq_attn_switches_from_env() {
    fq_attn_switches s;
    s.rows = fq_attn_env_int("FQ_ATTN_ROWS", -1);
    s.mfma = fq_attn_env_int("FQ_ATTN_MFMA", 1) != 0;
    s.mfma16 = fq_attn_env_int("FQ_ATTN_MFMA16", 0) != 0;          s.mfma16h = fq_attn_env_int("FQ_ATTN_MFMA16H", 0) != 0;
    s.mfma16_maxkv = fq_attn_env_int("FQ_ATTN_MFMA16_MAXKV", 4096);
    s.flash = fq_attn_env_int("FQ_ATTN_FLASH", 1) != 0;            s.flash_long = fq_attn_env_int("FQ_ATTN_FLASH_LONG", 1) != 0;
    s.flash_tab = fq_attn_env_int("FQ_ATTN_FLASH_TAB", 1) != 0;    s.keep = fq_attn_env_int("FQ_ATTN_KEEP", 1) != 0;
    s.persist = fq_attn_env_int("FQ_ATTN_PERSIST", 1) != 0;        s.pack_min_n = fq_attn_env_int("FQ_ATTN_PACK_MIN_N", 256);
    s.scratch = fq_attn_env_int("FQ_ATTN_SCRATCH", 1) != 0;        s.scratch_gb = fq_attn_env_int("FQ_ATTN_SCRATCH_GB", 4);
    s.dbg = fq_attn_env_int("FQ_ATTN_DBG", 0);
    return s;
}
inline const fq_attn_switches & fq_attn_sw() { static const fq_attn_switches s = fq_attn_switches_from_env(); return s; }
static inline size_t fq_attn_scratch_cap(const fq_attn_switches & sw) { return (size_t) sw.scratch_gb << 30; }

// the process modes a plan depends on
struct fq_attn_mode {
    bool f64;                      // fq_attn_set_f64 (ggml_hip_reference_order != 0): the two dot products accumulate in f64 -- never the matrix pipe
    int  form;                     // fq_attn_set_form: 0 default, 1 k_attention_flash, 32 k_attention_mfma, 16 k_attention_mfma16, 17 k_attention_mfma16h
};
// the mode a launch plans with: a form set by fq_attn_set_form, else the environment's (FQ_ATTN_MFMA16H / FQ_ATTN_MFMA16)
static inline fq_attn_mode fq_attn_mode_of(bool f64, int set_form, const fq_attn_switches & sw) {
    return fq_attn_mode{ f64, set_form ? set_form : (sw.mfma16h ? 17 : (sw.mfma16 ? 16 : 0)) };
}

enum fq_attn_family {
    FQ_AF_REFUSE_HEAD_DIM = 0,   // head_dim != 64: message, exit
    FQ_AF_REFUSE_KEYS,           // one score row does not fit the CU's 160 KiB of LDS: message, exit
    FQ_AF_ONE_ROW,               // k_attention: one workgroup per (head, token)
    FQ_AF_ROWS_LDS,              // k_attention_rows<R>: R tokens per workgroup, their score rows in LDS
    FQ_AF_ROWS_SCRATCH,          // k_attention_rows<4>: the score rows in the workgroup's slice of the global scratch
    FQ_AF_FLASH,                 // k_attention_flash<TAB, nt, PACKED, keep, lng>: 32-token tiles, fp16 probabilities in LDS
    FQ_AF_MFMA16,                // k_attention_mfma16: 16-token tiles, f32 scores in LDS
    FQ_AF_MFMA16H,               // k_attention_mfma16h: 16-token tiles, fp16 probabilities in LDS
    FQ_AF_MFMA_SCRATCH,          // k_attention_mfma: 32-token tiles, the scores in the global scratch
};
struct fq_attn_plan {
    int      family;
    int      R;                    // query tokens per workgroup
    int      nt;                   // FLASH: key tiles of the LDS rows' compile-time pitch (16, 32, 64, 74)
    bool     keep, lng;            // FLASH: the KEEP / LONG instantiation
    bool     packed;               // FLASH: k_attn_pack_k runs first, into scratch_bytes of scratch
    int      nt_total;             // FLASH, packed: key tiles of the launch (the grid of k_attn_pack_k, the kernel's clamp); else 0
    bool     ctx_tab;              // FLASH: where the caller passes no exp table the library's own is used (exp() is a table gather whenever there is a table)
    bool     persistent;           // FLASH: one workgroup per CU, items from a counter the launcher zeroes
    int      dbg;                  // FLASH: FQ_ATTN_DBG
    unsigned grid_x, grid_y, block;
    size_t   lds;                  // dynamic LDS bytes
    int      pitch;                // elements between score rows (LDS or scratch)
    size_t   scratch_bytes;        // global scratch the launch needs (never more than scratch_cap)
};

// ---- LDS and scratch arithmetic, each formula once
constexpr size_t FQ_ATTN_LDS_MAX = 160 * 1024;
constexpr size_t FQ_ATTN_ROWS_FIXED = 16 * 4 + 16 * 64 * 8;      // k_attention / k_attention_rows: 16 floats + 16 x 64 doubles of reduction space in front of the score rows
static inline int    fq_attn_row_pitch(int max_n_kv) { return (max_n_kv + 3) & ~3; }
static inline size_t fq_attn_rows_lds(int R, int max_n_kv) { return FQ_ATTN_ROWS_FIXED + (size_t) R * (size_t) fq_attn_row_pitch(max_n_kv) * 4; }
static inline size_t fq_attn_one_row_lds(int max_n_kv) { return fq_attn_rows_lds(1, max_n_kv); }
static inline bool   fq_attn_one_row_fits(int max_n_kv) { return fq_attn_one_row_lds(max_n_kv) <= FQ_ATTN_LDS_MAX; }
// R rows in LDS beside enough other workgroups
static inline bool   fq_attn_rows_fit(int R, int max_n_kv) { return fq_attn_rows_lds(R, max_n_kv) <= 150 * 1024; }
// tokens per workgroup: more tokens re-use a key tile more often, but their score rows (n_kv floats each) sit in LDS and leave fewer workgroups per CU. Measured on
// Falcon-7B, ms per block for 4 / 2 / 1 tokens: 2048-token prompt 2.08 / 2.21 / (f64: 3.7); 4096 tokens 8.65 / 8.36; 8192 tokens 52.9 / 36.1 / 41.9 -> 4 while that
// keeps >= 3 workgroups per CU (n_kv <= ~3000), else 2
static inline bool   fq_attn_rows4_default(int max_n_kv) { return fq_attn_rows_lds(4, max_n_kv) <= 56 * 1024; }
// ... and beyond ~3000 keys: 4 tokens per workgroup with the score rows in the global scratch instead of 2 with them in LDS (8192-token prompt: 32 ms per block
// against 36-40; 8 tokens per workgroup: 38). The scratch is N x H x n_kv floats -- 1.2 GB for a 512-token batch at 8192 keys
static inline size_t fq_attn_rows4_scratch_bytes(int N, int H, int max_n_kv) { return (size_t)((N + 3) / 4) * (size_t) H * 4 * ((size_t) fq_attn_row_pitch(max_n_kv) * 4); }
// k_attention_mfma: 32 score rows of whole key tiles per (head, query tile)
static inline int    fq_attn_tile_pitch(int max_n_kv) { return (max_n_kv + 31) & ~31; }
static inline size_t fq_attn_mfma_scratch_bytes(int N, int H, int max_n_kv) { return (size_t)((N + 31) / 32) * (size_t) H * 32 * (size_t) fq_attn_tile_pitch(max_n_kv) * 4; }
// k_attention_mfma16: [16][pitch] f32 scores, row maxima of 8 waves, 16 inverses, the exchange of 4 dim tiles (pitch: 4 floats beyond whole tiles)
static inline int    fq_attn_mfma16_pitch(int max_n_kv) { return fq_attn_tile_pitch(max_n_kv) + 4; }
static inline size_t fq_attn_mfma16_lds(int max_n_kv) { return ((size_t) 16 * fq_attn_mfma16_pitch(max_n_kv) + 8 * 16 + 16 + 4 * 4 * 64) * 4; }
// k_attention_mfma16h: row maxima (f32) and sums (f64) of 8 waves, the exchange, [16][pitch] fp16 probabilities (pitch in uint16 elements)
static inline int    fq_attn_mfma16h_pitch(int max_n_kv) { return fq_attn_tile_pitch(max_n_kv) + 8; }
static inline size_t fq_attn_mfma16h_lds(int max_n_kv) { return (8 * 16) * 4 + (8 * 16) * 8 + (4 * 4 * 64) * 4 + (size_t) 16 * fq_attn_mfma16h_pitch(max_n_kv) * 2; }
constexpr size_t FQ_ATTN_MFMA16_LDS_MAX = 158 * 1024;
// k_attention_flash: [32][32 nt + 8] fp16 probabilities, row maxima and sums of 8 waves, the exchange of 2 dim halves, the next-item word
static inline size_t fq_attn_flash_lds(int nt) { return (size_t) 32 * (size_t)(32 * nt + 8) * 2 + 8 * 32 * 4 + 8 * 32 * 8 + 2 * 16 * 64 * 4 + 16; }
// LDS rows for 16, 32, 64 or 74 key tiles (512, 1024, 2048, 2368 keys): the instantiations of the compile-time pitch. 64 is the KEEP form's largest (8 tiles x 16
// score registers per wave); 65-74 tiles (and 33-64 with FQ_ATTN_KEEP=0) run the three-pass form at pitch 74; beyond 74 tiles the LONG form in chunks of 64 tiles
// (FQ_ATTN_FLASH_LONG=0: no flash form there -- nt 0 --, as before round 6)
struct fq_attn_flash_pitch { int nt; bool keep, lng; };
static inline fq_attn_flash_pitch fq_attn_flash_pitch_of(int max_n_kv, const fq_attn_switches & sw) {
    const int tiles = (max_n_kv + 31) >> 5;
    if (tiles <= 16) return { 16, sw.keep, false };
    if (tiles <= 32) return { 32, sw.keep, false };
    if (tiles <= 64 && sw.keep) return { 64, true, false };
    if (tiles <= 74) return { 74, false, false };
    if (sw.flash_long) return { 64, false, true };
    return { 0, false, false };
}
static inline bool   fq_attn_flash_fits(int max_n_kv, const fq_attn_switches & sw) { return fq_attn_flash_pitch_of(max_n_kv, sw).nt != 0; }
// bytes of the packed keys (and values) a launch of this size wants (k_attn_pack_k): prompts of FQ_ATTN_PACK_MIN_N (default 256) tokens and more
static inline size_t fq_attn_pack_bytes(int N, int HKV, int max_n_kv, const fq_attn_switches & sw) {
    return N >= sw.pack_min_n ? (size_t) HKV * (size_t)((max_n_kv + 31) >> 5) * 8192 * (FQ_ATTN_PACK_V ? 2 : 1) : 0;
}

// ---- the plan of one launch. lockstep: the N rows are N independent sequences (seq_stride != 0). scratch_cap: the largest scratch the caller can hand over -- a
// context's own buffer (never grown inside a launch), or fq_attn_scratch_cap(sw) for the op-level API's process-wide one
static inline fq_attn_plan fq_attn_plan_of(int N, int H, int HKV, int D, int max_n_kv, bool lockstep, const fq_attn_mode & mode, const fq_attn_switches & sw,
                                           int n_cu, size_t scratch_cap) {
    fq_attn_plan p = {};
    p.family = D != 64 ? FQ_AF_REFUSE_HEAD_DIM : (!fq_attn_one_row_fits(max_n_kv) ? FQ_AF_REFUSE_KEYS : FQ_AF_ONE_ROW);
    if (p.family != FQ_AF_ONE_ROW) return p;
    const int force = sw.rows;
    p.grid_x = (unsigned) H;
    if (sw.mfma && N >= 32 && !mode.f64 && !lockstep && force < 0) {
        // the f32 matrix pipe: k_attention_flash while its LDS rows fit; forms 16 / 17 (measured slower than the scratch form at 2048 tokens, see k_attention_mfma16h)
        // keep the score rows of 16 query tokens in LDS while they fit (~2400 keys); else 32 tokens per workgroup and the global scratch
        const fq_attn_flash_pitch fp = fq_attn_flash_pitch_of(max_n_kv, sw);
        if ((mode.form == 1 || (mode.form == 0 && sw.flash)) && fp.nt) {
            const size_t pk = fq_attn_pack_bytes(N, HKV, max_n_kv, sw);
            const int n_items = H * ((N + 31) / 32);
            p.family = FQ_AF_FLASH; p.R = 32; p.nt = fp.nt; p.keep = fp.keep; p.lng = fp.lng;
            p.packed = pk && pk <= scratch_cap; p.scratch_bytes = p.packed ? pk : 0; p.nt_total = p.packed ? (max_n_kv + 31) >> 5 : 0;
            // pass B reads exp() from the fp16 table even when the in-kernel formula is verified: ~25 VALU instructions per score make the pass VALU-bound (measured in
            // the model: 2048-token prompt 110.6 ms with the formula, the table gather rides on the vector cache under the matrix instructions)
            p.ctx_tab = sw.flash_tab;
            p.persistent = sw.persist && n_items >= 4 * n_cu;          // persistent workgroups where there are rounds enough to amortise over
            p.dbg = sw.dbg;
            p.grid_x = (unsigned)(p.persistent ? n_cu : n_items); p.grid_y = 1; p.block = 512; p.lds = fq_attn_flash_lds(fp.nt); p.pitch = 32 * fp.nt + 8;
            return p;
        }
        if (mode.form == 16 && fq_attn_mfma16_lds(max_n_kv) <= FQ_ATTN_MFMA16_LDS_MAX && max_n_kv <= sw.mfma16_maxkv) {
            p.family = FQ_AF_MFMA16; p.R = 16; p.grid_y = (unsigned)((N + 15) / 16); p.block = 512; p.lds = fq_attn_mfma16_lds(max_n_kv); p.pitch = fq_attn_mfma16_pitch(max_n_kv);
            return p;
        }
        if (mode.form == 17 && fq_attn_mfma16h_lds(max_n_kv) <= FQ_ATTN_MFMA16_LDS_MAX) {
            p.family = FQ_AF_MFMA16H; p.R = 16; p.grid_y = (unsigned)((N + 15) / 16); p.block = 512; p.lds = fq_attn_mfma16h_lds(max_n_kv); p.pitch = fq_attn_mfma16h_pitch(max_n_kv);
            return p;
        }
        // (a 128-token-per-workgroup form with the key / value tiles shared through LDS was built and measured: 124 ms against 112 ms for a 2048-token Falcon-7B
        // prompt -- a barrier per tile and idle waves at the causal edge cost more than the L2 traffic it saves)
        if (fq_attn_mfma_scratch_bytes(N, H, max_n_kv) <= scratch_cap) {
            p.family = FQ_AF_MFMA_SCRATCH; p.R = 32; p.grid_y = (unsigned)((N + 31) / 32); p.block = 256; p.lds = 0; p.pitch = fq_attn_tile_pitch(max_n_kv);
            p.scratch_bytes = fq_attn_mfma_scratch_bytes(N, H, max_n_kv);
            return p;
        }
    }
    // the rows forms. Independent sequences share no key tile: one token per workgroup
    int R = (N >= 4 && fq_attn_rows4_default(max_n_kv)) ? 4 : ((N >= 2 && fq_attn_rows_fit(2, max_n_kv)) ? 2 : 1);
    if (force == 0 || lockstep) R = 1;
    else if ((force == 8 || force == 4) && N >= 4 && fq_attn_rows_fit(force, max_n_kv)) R = force;
    else if (force == 2 && N >= 2 && fq_attn_rows_fit(2, max_n_kv)) R = 2;
    p.block = 256; p.pitch = fq_attn_row_pitch(max_n_kv);
    if (sw.scratch && force < 0 && R == 2 && N >= 4 && !lockstep && fq_attn_rows4_scratch_bytes(N, H, max_n_kv) <= scratch_cap) {
        p.family = FQ_AF_ROWS_SCRATCH; p.R = 4; p.grid_y = (unsigned)((N + 3) / 4); p.lds = FQ_ATTN_ROWS_FIXED; p.scratch_bytes = fq_attn_rows4_scratch_bytes(N, H, max_n_kv);
        return p;
    }
    p.family = R > 1 ? FQ_AF_ROWS_LDS : FQ_AF_ONE_ROW; p.R = R; p.grid_y = (unsigned)((N + R - 1) / R); p.lds = fq_attn_rows_lds(R, max_n_kv);
    return p;
}

// ---- the scratch a context allocates once, at context_create, for every launch of up to n_batch tokens and n_ctx keys: the largest plan's, capped. 0: no launch
// of that size uses a scratch.
// THE GAP (ADVICE.md's second finding, open): this sizes for the DEFAULT plan of the (n_batch, n_ctx) corner only. With the LONG form k_attention_flash fits every
// n_ctx, so a context of n_batch >= 32 gets the packed keys' bytes and nothing else -- while fq_attn_plan_of, for the same context in f64 order (reference orders
// 1 / 2) or for a batch of 4..31 tokens beyond ~3000 keys, wants fq_attn_rows4_scratch_bytes, finds scratch_cap too small and plans 2 rows in LDS (36-40 against
// 32 ms per block at 8192 keys). Results are the same; tests/test_attn_forms_cpu.py::test_context_scratch_gap_as_it_stands pins those plans, so the fix shows as a
// table change.
static inline size_t fq_attn_scratch_need(int n_batch, int H, int n_ctx, int HKV, const fq_attn_switches & sw) {
    if (n_batch < 4) return 0;
    if (n_batch >= 32 && sw.flash && fq_attn_flash_fits(n_ctx, sw)) return fq_attn_pack_bytes(n_batch, HKV, n_ctx, sw);      // k_attention_flash: only the packed keys
    const size_t a = n_batch >= 32 ? fq_attn_mfma_scratch_bytes(n_batch, H, n_ctx) : 0;      // k_attention_mfma: only contexts too long for k_attention_flash's LDS rows
    const size_t b = !fq_attn_rows4_default(n_ctx) ? fq_attn_rows4_scratch_bytes(n_batch, H, n_ctx) : 0;      // 4 tokens per workgroup, once their rows leave LDS
    const size_t need = a > b ? a : b, cap = fq_attn_scratch_cap(sw);
    // beyond the cap the context still gets cap bytes: every launch is planned with its own byte count, so batches at low n_past (whose score rows are short) keep the
    // MFMA / 4-row forms in a context whose (n_batch, n_ctx) corner would not fit
    return need > cap ? cap : need;
}

// a plan as integers (the harness and ggml_hip_debug_attention_plan share the layout): family, R, nt, keep, long, packed, nt_total, ctx_tab, persistent, grid x, grid y,
// block, LDS bytes, pitch, scratch bytes, dbg
constexpr int FQ_ATTN_PLAN_INTS = 16;
static inline void fq_attn_plan_ints(const fq_attn_plan & p, int64_t * o) {
    const int64_t v[FQ_ATTN_PLAN_INTS] = { p.family, p.R, p.nt, p.keep, p.lng, p.packed, p.nt_total, p.ctx_tab, p.persistent, p.grid_x, p.grid_y, p.block,
                                           (int64_t) p.lds, p.pitch, (int64_t) p.scratch_bytes, p.dbg };
    for (int i = 0; i < FQ_ATTN_PLAN_INTS; ++i) o[i] = v[i];
}
