// Host build of ggllm.cpp_amd/csrc/fq_attn_forms.h for tests/test_attn_forms_cpu.py: the prompt attention's plan as fq_launch_attention runs it, with the switches the
// test names (never the environment's): sw[14] = rows, mfma, mfma16, mfma16h, mfma16_maxkv, flash, flash_long, flash_tab, keep, persist, pack_min_n, scratch,
// scratch_gb, dbg.
#include "fq_attn_forms.h"

static fq_attn_switches sw_of(const int * v) {
    fq_attn_switches s;
    s.rows = v[0]; s.mfma = v[1] != 0; s.mfma16 = v[2] != 0; s.mfma16h = v[3] != 0; s.mfma16_maxkv = v[4]; s.flash = v[5] != 0; s.flash_long = v[6] != 0;
    s.flash_tab = v[7] != 0; s.keep = v[8] != 0; s.persist = v[9] != 0; s.pack_min_n = v[10]; s.scratch = v[11] != 0; s.scratch_gb = v[12]; s.dbg = v[13];
    return s;
}

extern "C" {

// the defaults, in sw[]'s order
void atf_default_switches(int * v) {
    const fq_attn_switches s;
    const int d[14] = { s.rows, s.mfma, s.mfma16, s.mfma16h, s.mfma16_maxkv, s.flash, s.flash_long, s.flash_tab, s.keep, s.persist, s.pack_min_n, s.scratch, s.scratch_gb, s.dbg };
    for (int i = 0; i < 14; ++i) v[i] = d[i];
}
// out[FQ_ATTN_PLAN_INTS]: fq_attn_plan_ints. scratch_cap < 0: the switches' cap (the op-level API)
void atf_plan(int N, int H, int HKV, int D, int max_n_kv, int lockstep, int f64, int set_form, const int * sw, int n_cu, long long scratch_cap, long long * out) {
    const fq_attn_switches s = sw_of(sw);
    const fq_attn_plan p = fq_attn_plan_of(N, H, HKV, D, max_n_kv, lockstep != 0, fq_attn_mode_of(f64 != 0, set_form, s), s, n_cu,
                                           scratch_cap < 0 ? fq_attn_scratch_cap(s) : (size_t) scratch_cap);
    int64_t o[FQ_ATTN_PLAN_INTS];
    fq_attn_plan_ints(p, o);
    for (int i = 0; i < FQ_ATTN_PLAN_INTS; ++i) out[i] = o[i];
}
long long atf_scratch_need(int n_batch, int H, int n_ctx, int HKV, const int * sw) { return (long long) fq_attn_scratch_need(n_batch, H, n_ctx, HKV, sw_of(sw)); }
long long atf_one_row_lds(int max_n_kv) { return (long long) fq_attn_one_row_lds(max_n_kv); }
int atf_one_row_fits(int max_n_kv) { return fq_attn_one_row_fits(max_n_kv); }

}
