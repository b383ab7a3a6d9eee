// Host build of ggllm.cpp_amd/csrc/fq_mm_forms.h for tests/test_mm_forms_cpu.py: the mat-mul form rules as the launchers run them, with the default switches
// (never the environment's) and the modes the test names.
#include "fq_mm_forms.h"

static fq_mm_mode mode_of(int ref_order, int sequential, int force_gemv, int forced_cfg) {
    fq_mm_mode md;
    md.ref_order = ref_order; md.sequential = sequential != 0; md.force_gemv = force_gemv != 0; md.forced_cfg = forced_cfg;
    return md;
}
static const fq_mm_switches SW{};

extern "C" {

// out[9] = family, S, cfg, passes, pass_w, wg_rows, tile_cols, stream_kind, uses_scratch
void mmf_form(int type, long long M, long long K, long long N, int n_cu, int ref_order, int sequential, int force_gemv, int forced_cfg, int from3, int * out) {
    const fq_mm_form f = fq_mm_form_of(fq_mm_mat_make(type, M, K), N, n_cu, mode_of(ref_order, sequential, force_gemv, forced_cfg), SW, from3 != 0);
    out[0] = f.family; out[1] = f.S; out[2] = f.cfg; out[3] = f.passes; out[4] = f.pass_w; out[5] = f.wg_rows; out[6] = f.tile_cols; out[7] = f.stream_kind; out[8] = f.uses_scratch;
}
// out[FQ_MM_KEY_LEN = 8]: the launch key of the same call (fq_mm_launch_key: family, S, passes > 1, stream kind, four facts of the form)
void mmf_launch_key(int type, long long M, long long K, long long N, int n_cu, int ref_order, int sequential, int force_gemv, int forced_cfg, int from3, int * out) {
    fq_mm_launch_key(fq_mm_mat_make(type, M, K), N, n_cu, mode_of(ref_order, sequential, force_gemv, forced_cfg), SW, from3 != 0, out);
}
// the tile cfg alone, whatever form takes the shape (what fq_launch_gemm falls back to), and the cfg -> (S, rows, columns) table
int mmf_tile_cfg(int type, long long M, long long N, int n_cu, int sequential, int forced_cfg) {
    return fq_mm_tile_cfg(type, M, N, n_cu, mode_of(0, sequential, 0, forced_cfg), SW);
}
void mmf_cfg_shape(int cfg, int * out) { out[0] = fq_mm_cfg_split(cfg); out[1] = fq_mm_cfg_wg_rows(cfg); out[2] = fq_mm_cfg_tile_cols(cfg); }
long long mmf_gemm_wgs(int type, long long M, long long K, long long N, int n_cu, int forced_cfg) {
    return fq_mm_gemm_wgs(fq_mm_mat_make(type, M, K), N, n_cu, mode_of(0, 0, 0, forced_cfg), SW);
}
int mmf_pair_split(int type, long long M0, long long M1, long long K, long long N, int n_cu, int ref_order, int forced_cfg) {
    return fq_mm_pair_split(fq_mm_mat_make(type, M0, K), fq_mm_mat_make(type, M1, K), fq_desc(type).act_type, K, N, n_cu, mode_of(ref_order, ref_order != 0, 0, forced_cfg), SW);
}
int mmf_out2_legacy(int type, long long M, long long K_wo, long long K_down, long long N, int n_cu, int ref_order, int forced_cfg) {
    const int at = fq_desc(type).act_type;
    return fq_mm_out2_legacy_ok(fq_mm_mat_make(type, M, K_wo), fq_mm_mat_make(type, M, K_down), at, at, N, n_cu, mode_of(ref_order, ref_order != 0, 0, forced_cfg), SW);
}
int mmf_q4k_fused_ok(long long N, long long min_cols, int ref_order, int forced_cfg) { return fq_mm_q4k_fused_ok(N, min_cols, mode_of(ref_order, ref_order != 0, 0, forced_cfg), SW); }
int mmf_q4k_fused_passes(int type, long long M, long long K, long long N, int ref_order, int forced_cfg) {
    return fq_mm_q4k_fused_passes(fq_mm_mat_make(type, M, K), N, mode_of(ref_order, ref_order != 0, 0, forced_cfg), SW);
}
int mmf_q4k_shape(int type, long long M, long long K) { return fq_mm_q4k_shape(fq_mm_mat_make(type, M, K), SW); }
int mmf_cols_max_n(int type, long long M, long long K) { return fq_mm_cols_max_n(fq_mm_mat_make(type, M, K), SW); }
// a block of n_embd E, qkv_rows rows of Wqkv and n_ff FF: would a matrix of each branch of the two-stream form write the shared scratch at N columns?
int mmf_par2_clash(int type, long long E, long long qkv_rows, long long FF, long long N, int n_cu) {
    return fq_mm_par2_scratch_clash(fq_mm_mat_make(type, qkv_rows, E), fq_mm_mat_make(type, E, E), fq_mm_mat_make(type, FF, E), fq_mm_mat_make(type, E, FF), N, n_cu, mode_of(0, 0, 0, -1), SW);
}

}
