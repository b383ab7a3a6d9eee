// falcon_stage.hip -- launch_stage: every launch of one eval of a stage (the op sequence: falcon_hip.hip's header), and the predicates
// that say which list an N = 1 step takes. Host code only; the kernels are the kernels_* units'.
#include "falcon_ctx.h"
using namespace fq_drv;

// the image view of `buf` for the activations that weight `w` consumes
static fq_act act_for(uint8_t * buf, const fq_weight & w, int64_t cols) {
    fq_act a{}; a.type = w.type == FQ_F16 ? (int) FQ_F16 : fq_desc(w.type).act_type; a.K = w.K; a.ncols = cols; a.base = buf; return a;
}

static bool stage_uniform(const falcon_hip_model * m) {
    for (const layer_weights & L : m->layers) if (L.qkv.type != L.up.type || L.down.type != L.wo.type) return false;
    return true;
}
// THE predicate for "an N = 1 step of this context runs the fused decode kernels" -- launch_stage, the greedy sampler and
// the pipeline step all ask here, so the sampler reads the per-workgroup argmax candidates exactly when the fused lm_head
// wrote them. The fused kernels are instantiated per weight format (a model that mixes formats inside a block takes the
// op list) and implement the default summation order only (ggml_hip_reference_order -> op list).
// Round 6: the FAST reference order (ggml_hip_reference_order(2)) has the fused launches too, for stages of one legacy format (fq_ref_chain.h).
static bool stage_legacy(const falcon_hip_model * m) {
    auto leg = [](int t) { return t == FQ_Q4_0 || t == FQ_Q4_1 || t == FQ_Q5_0 || t == FQ_Q5_1 || t == FQ_Q8_0; };
    if (m->layers.empty() || m->hp.n_embd % 32 || m->hp.n_ff % 32) return false;
    const int t = m->layers[0].qkv.type;
    for (const layer_weights & L : m->layers) if (L.qkv.type != t || L.up.type != t || L.down.type != t || L.wo.type != t) return false;
    if (m->last_stage() && !leg(m->lm_head.type)) return false;
    return leg(t);
}
bool fq_drv::stage_fused_ref(const falcon_hip_context * c) {       // N = 1 steps run the fused launches in the reference's association
    return c->fused_decode && fq_reference_fast() && stage_legacy(c->m) && !c->two_phase && !c->dual_stream;
}
bool fq_drv::stage_fused(const falcon_hip_context * c) {
    if (stage_fused_ref(c)) return true;
    return c->fused_decode && stage_uniform(c->m) && !stage_has_f16(c->m) && !fq_reference_order() && !fq_attn_f64();
}
// ------------------------------------------------------------------------------------------------ one eval
// Launches every kernel of this stage for N tokens. Inputs already in place: tokens_dev (first stage) or x, and
// n_past_dev. max_n_kv bounds n_past + N for LDS sizing. pos_stride 1 (lock-step contexts only): a ragged step, row t at
// position pos_dev[t] (max_n_kv > every one of them); 0: every row at n_past_dev.
// verify_limit > 0 (plain contexts, 2 <= N <= 16: a draft-and-verify pass, falcon_hip_decode_spec): the N rows are the positions n_past_dev + t of the one cache, as
// in a prompt batch, but a row whose position would be >= verify_limit (n_ctx) appends nothing and is not attended for (kernels_block.hip: the verify launches);
// and 2..4 rows take the column mat-vec launches a lock-step context of as many sequences takes -- one pass over the weights, every row the bits of the single row.
// lock-step contexts (and verify passes) of up to this many rows run the column mat-vec kernels in chunks of 4: fq_mm_cols_max_n (fq_mm_forms.h), from the model's first Wqkv
static int cols_max_n(const falcon_hip_model * m) { return m->layers.empty() ? 4 : fq_mm_cols_max_n(fq_mm_mat_of(m->layers[0].qkv), fq_mm_sw()); }
// ---- the fused single-token path of launch_stage
static void launch_stage_token(falcon_hip_context * c, int max_n_kv, hipStream_t st) {
    falcon_hip_model * m = c->m;
    const falcon_hip_hparams & hp = m->hp;
    hip_context & hc = fq_ctx();
    const int64_t E = hp.n_embd, D = 64, H = hp.n_head, HKV = hp.n_head_kv, FF = hp.n_ff;
    const int64_t n_caches = c->n_seq > 0 ? c->n_seq : 1;
    // ---- fused single-token path (kernels_decode.hip), bit-identical to the op list below. Per block, by mode:
    //   3 launches  k_gemv_ln | k_attn_decode | k_gemv_out
    //   2 launches  k_gemv_ln | k_attn_out                        (attention inside the output mat-vec launch)
    //   1 launch    k_attn_out_ln = k_attn_out of block l + k_gemv_ln of block l+1 (or ln_f + lm_head) as a second phase
    const bool prof = fq_prof_active();
    const bool dual = c->dual_stream && !prof;
    const bool ref = stage_fused_ref(c);                    // the reference's association on the same launches (fq_ref_chain.h)
    auto ln_args = [&](size_t li) {
        const layer_weights & L = m->layers[li];
        const int ff_act = fq_desc(L.down.type).act_type;
        const bool quant_epi = (ff_act == FQ_Q8_0 || ff_act == FQ_Q8_1);
        fq_gemv_ln_args ga{};
        ga.x = c->x; ga.E = E; ga.nseg = 2; ga.gelu_table = hc.gelu_table; ga.dbg = hc.dbg_stamps;
        ga.epoch_word = c->merged_attn_out ? c->sync_words : nullptr;
        if (c->merged_attn_out) { ga.n_past_ptr = c->n_past_dev; ga.rope_cs = c->rope_cs; ga.rope_cur = (float *)(c->sync_words + 16); }
        ga.seg[0] = { L.qkv, hp.two_norms ? L.ln2_w : L.ln_w, hp.two_norms ? L.ln2_b : L.ln_b, FQ_LNEPI_STORE, c->qkv, nullptr, 0, 0 };
        ga.seg[1] = { L.up, L.ln_w, L.ln_b, quant_epi ? FQ_LNEPI_GELU_QUANT : FQ_LNEPI_GELU_STORE, c->up, c->buf_ff, ff_act, 0 };
        return ga;
    };
    auto head_args = [&]() {
        fq_gemv_ln_args ga{};
        ga.x = c->x; ga.E = E; ga.nseg = 1; ga.gelu_table = hc.gelu_table;
        ga.epoch_word = c->merged_attn_out ? c->sync_words : nullptr;
        ga.seg[0] = { m->lm_head, m->out_norm_w, m->out_norm_b, FQ_LNEPI_STORE, c->logits_dev, nullptr, 0, 0 };
        ga.argmax_val = c->argmax_val; ga.argmax_idx = c->argmax_idx;
        return ga;
    };
    bool ln_done = false;                                   // this block's k_gemv_ln already ran as the previous launch's second phase
    bool head_done = false;
    for (size_t li = 0; li < m->layers.size(); ++li) {
        const layer_weights & L = m->layers[li];
        if (c->keep_hidden) HIP_CHECK(hipMemcpyAsync(c->hidden_dev + li * (size_t) E, c->x, (size_t) E * 4, hipMemcpyDeviceToDevice, st));
        const int ff_act = fq_desc(L.down.type).act_type;
        const bool quant_epi = (ff_act == FQ_Q8_0 || ff_act == FQ_Q8_1);
        const fq_gemv_ln_args ga = ln_args(li);
        if (dual) {
            // the MLP-up mat-vec only needs x: run it on the side stream while QKV + attention run on the main one
            fq_gemv_ln_args gu = ga; gu.nseg = 1; gu.seg[0] = ga.seg[1]; gu.seg[0].block_begin = 0;
            fq_gemv_ln_args gq = ga; gq.nseg = 1;
            HIP_CHECK(hipEventRecord(c->ev_fork[li], st));
            HIP_CHECK(hipStreamWaitEvent(c->side, c->ev_fork[li], 0));
            fq_launch_gemv_ln(gu, hc.n_cu, c->side);
            if (!quant_epi) fq_launch_quantize_act(c->up, FF, act_for(c->buf_ff, L.down, 1), c->side);
            HIP_CHECK(hipEventRecord(c->ev_join[li], c->side));
            fq_launch_gemv_ln(gq, hc.n_cu, st);
        } else if (!ln_done) {
            if (prof) fq_prof_open(st);
            bool ring = false;
            if (c->ring_ln && quant_epi) ring = fq_launch_gemv_ln_ring(ga, c->sync_words + 1, hc.n_cu, st, ref);
            else if (c->ring_ln && !ref) ring = fq_launch_ringk_ln(ga, c->sync_words + 1, hc.n_cu, st);      // k-quants: GELU stored as f32
            if (!ring) fq_launch_gemv_ln(ga, hc.n_cu, st, ref);
            if (prof) fq_prof_close(st, (double)(L.qkv.bytes + L.up.bytes));
        }
        ln_done = false;
        float * kc = c->k_cache + li * (size_t) n_caches * c->n_ctx * HKV * D;
        float * vc = c->v_cache + li * (size_t) n_caches * c->n_ctx * HKV * D;
        const int att_act = fq_desc(L.wo.type).act_type;
        const bool att_q = (att_act == FQ_Q8_0 || att_act == FQ_Q8_1);      // the head's 64 outputs = two 32-blocks
        fq_gemv_out_args go{ L.down, L.wo, c->buf_ff, c->att, att_q ? c->buf_att : nullptr, c->x, c->x,
                             hc.dbg_stamps ? hc.dbg_stamps + 4096 * 8 : nullptr };
        if (dual) HIP_CHECK(hipStreamWaitEvent(st, c->ev_join[li], 0));
        // the merged attention + output launch: in the reference's association (ref), or with the next block's k_gemv_ln / the head as a second phase (next)
        auto attn_out = [&](bool in_ref_order, const fq_gemv_ln_args * next) {
            if (in_ref_order) return fq_launch_attn_out_ref(go, c->qkv, (int) H, (int) HKV, c->n_past_dev, max_n_kv, c->rope_cs, (const float *)(c->sync_words + 16),
                                                            kc, vc, hc.exp_table_attn, att_act, c->att_gran, c->sync_words, c->sync_words + 1, hc.n_cu, st);
            return fq_launch_attn_out(go, c->qkv, (int) H, (int) HKV, c->n_past_dev, max_n_kv, c->rope_cs, (const float *)(c->sync_words + 16),
                                      kc, vc, hc.exp_table_attn, att_act, c->att_gran, c->sync_words, c->sync_words + 1, hc.n_cu, st, next, next ? c->x_gran : nullptr);
        };
        // gelu(up) still f32 (k-quant consumers: a Q8_K block spans 256 rows, i.e. several workgroups of the launch above): quantized by its own launch
        // ahead of the merged form, or by extra workgroups of the attention launch (the rider) in the three-launch form
        bool ff_pending = !quant_epi && !dual;
        bool merged = false;
        if (ref && c->merged_attn_out) {
            // the merged launch in the reference's association; where its grid does not fit the chip: attention (f64 dots) + output launch below
            if (prof) fq_prof_open(st);
            merged = attn_out(true, nullptr);
            if (prof) { if (merged) fq_prof_close(st, (double)(L.down.bytes + L.wo.bytes)); else fq_prof_cancel(); }
        }
        const bool will_merge = !ref && c->merged_attn_out && !dual && fq_attn_out_fits(go, (int) H, max_n_kv, hc.n_cu);
        if (ff_pending && will_merge) { fq_launch_quantize_act(c->up, FF, act_for(c->buf_ff, L.down, 1), st); ff_pending = false; }
        if (will_merge) {
            // second phase: the next block's k_gemv_ln (its GELU output must be quantized in its epilogue: a separate
            // quantizer launch cannot sit between the phases), or ln_f + lm_head after the last block
            fq_gemv_ln_args next{}; bool have_next = false; double next_bytes = 0.0;
            if (c->two_phase && !c->keep_hidden) {
                if (li + 1 < m->layers.size()) {
                    const layer_weights & Ln = m->layers[li + 1];
                    const int a2 = fq_desc(Ln.down.type).act_type;
                    if (a2 == FQ_Q8_0 || a2 == FQ_Q8_1) { next = ln_args(li + 1); have_next = true; next_bytes = (double)(Ln.qkv.bytes + Ln.up.bytes); }
                } else if (m->last_stage() && !c->emb_mode) { next = head_args(); have_next = true; next_bytes = (double) m->lm_head.bytes; }      // (embeddings: the head stays a launch of its own, which falcon_hip_embed leaves out -- keep_hidden's precedent, for the last block only; c->x is whole behind either launch)
            }
            if (prof) fq_prof_open(st);
            if (have_next) {
                merged = attn_out(false, &next);
                if (merged) {
                    if (li + 1 < m->layers.size()) ln_done = true; else head_done = true;
                    if (prof) { fq_prof_close(st, (double)(L.down.bytes + L.wo.bytes) + next_bytes); }
                }
            }
            if (!merged) {
                merged = attn_out(false, nullptr);
                if (merged && prof) fq_prof_close(st, (double)(L.down.bytes + L.wo.bytes));
            }
            if (!merged && prof) fq_prof_cancel();
            if (!merged) { fprintf(stderr, "falcon-hip: the merged attention + output launch refused a shape fq_attn_out_fits accepted\n"); exit(1); }
        }
        if (!merged) {
            const fq_act a_ff1 = act_for(c->buf_ff, L.down, 1);
            if (ff_pending && fq_mm_sw().quant_rider && a_ff1.type == FQ_Q8_K && FF % 256 == 0) {
                // attention of the one sequence + the rider: k_attn_decode's code (k_attn_decode_seqs at one sequence), gelu(up)'s Q8_K image by extra workgroups
                fq_launch_attn_decode_seqs(c->qkv, 1, (int) H, (int) HKV, c->n_past_dev, max_n_kv, c->rope_cs, kc, vc, 0, hc.exp_table_attn,
                                           att_q ? nullptr : c->att, att_q ? c->buf_att : nullptr, att_act, (int64_t) fq_act_col_bytes(att_act, E), st, c->up, FF, &a_ff1);
                ff_pending = false;
            } else {
                if (ff_pending) { fq_launch_quantize_act(c->up, FF, a_ff1, st); ff_pending = false; }
                fq_launch_attn_decode(c->qkv, (int) H, (int) HKV, c->n_past_dev, max_n_kv, c->rope_cs, kc, vc, hc.exp_table_attn,
                                      att_q ? nullptr : c->att, att_q ? c->buf_att : nullptr, att_act, st, ref);
            }
            if (prof) fq_prof_open(st);
            if (ref) fq_launch_gemv_out(go, hc.n_cu, st, true);
            else if (!(c->ring_out && fq_launch_ring_out(go, c->sync_words + 1, hc.n_cu, st))) fq_launch_gemv_out(go, hc.n_cu, st);
            if (prof) fq_prof_close(st, (double)(L.down.bytes + L.wo.bytes));
        }
    }
    if (c->keep_hidden) {
        HIP_CHECK(hipMemcpyAsync(c->hidden_dev + m->layers.size() * (size_t) E, c->x, (size_t) E * 4, hipMemcpyDeviceToDevice, st));
        c->hidden_tokens = 1;
    }
    if (m->last_stage() && c->emb_mode) {                        // the ln_f row the fused head normalises for itself and drops
        fq_launch_layer_norm(c->x, E, 1, m->out_norm_w, m->out_norm_b, c->emb, st);
        if (c->emb_mode & FALCON_HIP_EMBED_POOL) fq_launch_embed_pool_accum(c->emb, 1, (int) E, c->pool_acc, c->pool_count, st);
        if (c->emb_no_head) return;
    }
    if (m->last_stage() && !head_done) {
        const fq_gemv_ln_args ga = head_args();
        if (prof) fq_prof_open(st);
        fq_launch_gemv_ln(ga, hc.n_cu, st, ref);
        if (prof) fq_prof_close(st, (double) m->lm_head.bytes);
    }
}

// ---- the batched path of launch_stage: one block
// what every launch of a block reads: its weights and caches, the four activation images, the rows and where they stand
struct stage_block {
    const layer_weights & L; size_t li; bool f16;      // f16: some matrix of the block is F16 -- the generic launches only: every fused / paired / two-stream form is per quantized format
    float * kc, * vc;
    fq_act a_qkv, a_up, a_att, a_ff;
    int N, max_n_kv;
    const int * seq_pos; int64_t seq_stride; int pos_stride, verify_limit;      // (launch_stage's header)
    hipStream_t st;
    const fq_mm_mode & md;                              // the process modes as of this launch_stage call (the form rules' input)
};
enum block_form { BLOCK_COLUMNS, BLOCK_TWO_STREAMS, BLOCK_GENERIC };
static fq_gemv_epi epi_store() { return fq_gemv_epi{ FQ_EPI_STORE, fq_ctx().gelu_table, nullptr, nullptr, 0 }; }
static fq_gemv_epi epi_gelu()  { return fq_gemv_epi{ FQ_EPI_GELU, fq_ctx().gelu_table, nullptr, nullptr, 0 }; }
static int64_t n_qkv(const falcon_hip_hparams & hp) { return ((int64_t) hp.n_head + 2 * hp.n_head_kv) * 64; }

// one mat-mul of a block (lock-step contexts: the k-quants' streaming forms from 3 sequences up, fq_mul_mat_q_acts_from3)
static void mm(const stage_block & b, const fq_weight & w, const fq_act & a, float * dst, int64_t ldd, const fq_gemv_epi & ep, hipStream_t st) {
    if (b.seq_stride) fq_mul_mat_q_acts_from3(w, a, b.N, dst, ldd, ep, st); else fq_mul_mat_q_acts(w, a, b.N, dst, ldd, ep, st);
}
// RoPE, KV append, attention and the image Wo takes, of all N rows.
//   lock-step sequences: one launch of the decode attention (k_attn_decode's code: the same bits as the three launches of a prompt), which also writes the
//     image for Q8_0 / Q8_1 consumers; ride: gelu(up)'s quantizer rides on that launch (Wup's GELU output exists already when Wqkv and Wup went in one launch)
//   a draft-and-verify pass: the verify launches (rows at or beyond verify_limit append nothing)
//   a prompt batch: rope + KV store, attention, quantize
static void block_attention(falcon_hip_context * c, const stage_block & b, bool ride) {
    const falcon_hip_hparams & hp = c->m->hp;
    hip_context & hc = fq_ctx();
    const int64_t E = hp.n_embd, FF = hp.n_ff;
    const int H = hp.n_head, HKV = hp.n_head_kv, D = 64;
    hipStream_t st = b.st;
    if (b.seq_stride && !fq_reference_order() && !fq_attn_f64()) {
        const bool att_q = (b.a_att.type == FQ_Q8_0 || b.a_att.type == FQ_Q8_1);
        fq_launch_attn_decode_seqs(c->qkv, b.N, H, HKV, b.seq_pos, b.max_n_kv, c->rope_cs, b.kc, b.vc, b.seq_stride, hc.exp_table_attn,
                                   att_q ? nullptr : c->att, att_q ? c->buf_att : nullptr, b.a_att.type, (int64_t) fq_act_col_bytes(b.a_att.type, E), st,
                                   ride ? c->up : nullptr, FF, ride ? &b.a_ff : nullptr, b.pos_stride);
        if (!att_q) fq_launch_quantize_act(c->att, E, b.a_att, st);
    } else if (b.verify_limit) {
        fq_launch_rope_kv_verify(c->qkv, b.N, H, HKV, D, c->n_past_dev, b.verify_limit, c->rope_cs, b.kc, b.vc, st);
        fq_launch_attention_verify(c->qkv, b.N, H, HKV, D, c->n_past_dev, b.verify_limit, b.kc, b.vc, hc.exp_table_attn, c->att, st);
        fq_launch_quantize_act(c->att, E, b.a_att, st);
    } else {
        fq_launch_rope_kv(c->qkv, b.N, H, HKV, D, b.seq_pos, c->rope_cs, b.kc, b.vc, st, b.seq_stride, b.pos_stride);
        fq_launch_attention(c->qkv, b.N, H, HKV, D, b.seq_pos, b.max_n_kv, b.kc, b.vc, hc.exp_table_attn, c->att, st, b.seq_stride, &c->att_scratch, b.pos_stride);
        fq_launch_quantize_act(c->att, E, b.a_att, st);
    }
}
// The LayerNorm(s) in front of a block (and the output norm) come out of the PREVIOUS block's residual-sum launch where that is a launch of its own (the short prompts'
// two-stream form): next_norm(li) = what block li (li == #blocks: the head) needs; false: no such launch for it
static bool next_norm(falcon_hip_context * c, size_t li, int N, fq_next_norm & nn) {
    falcon_hip_model * m = c->m;
    const int64_t E = m->hp.n_embd;
    nn = fq_next_norm{};
    if (li == m->layers.size()) {
        if (!m->last_stage()) return false;
        nn.w0 = m->out_norm_w; nn.b0 = m->out_norm_b; nn.a0 = act_for(c->buf_e, m->lm_head, N);
        return fq_add2_ln_ok(nn, E);
    }
    const layer_weights & Ln = m->layers[li];
    nn.w0 = Ln.ln_w; nn.b0 = Ln.ln_b; nn.a0 = act_for(c->buf_e, Ln.up, N);
    if (m->hp.two_norms) { nn.w1 = Ln.ln2_w; nn.b1 = Ln.ln2_b; nn.a1 = act_for(c->buf_e2, Ln.qkv, N); return fq_add2_ln_ok(nn, E); }
    return fq_desc(Ln.qkv.type).act_type == nn.a0.type && fq_add2_ln_ok(nn, E);      // (one norm, two activation families: two images of it -- launch_stage's own launches)
}

// Which form a block takes, decided up front from the form rules (fq_mm_forms.h) and the context's modes.
//   BLOCK_COLUMNS: 2..cols_max_n(m) lock-step sequences (or rows of a verify pass): the block's weights in TWO launches that serve every column (kernels_cols.hip),
//     the decode attention of all sequences in one launch between them -- same bits as the generic launches. In chunks of 4 columns; beyond cols_max_n one pass of
//     the streaming small-batch mat-mul (kernels_gemm_skinny.hip, N <= 16) is cheaper: measured on Falcon-7B Q4_0 3.6 ms per pass of 8 in two chunks, 4.0 ms for 12
//     and 4.1 ms for 16 in one pass (the 128-token tile GEMM beyond 16: 8.3-9.2 ms for any N up to 64)
//   BLOCK_TWO_STREAMS: batched evaluation (N > 4): a block's two branches -- {Wqkv, RoPE, attention, Wo} and {Wup + GELU, Wdown} -- only meet in
//     the residual sum, and three of the four mat-muls of a short prompt launch fewer workgroups than the chip has CUs (142
//     for a 4544-row matrix and 128 tokens). They run on two streams: the MLP branch on the side stream, its Wdown (whose
//     epilogue adds Wo's result and the residual) after the attention branch. Same kernels, same bits. Measured in one
//     process on the same resident Falcon-7B Q4_0 (scripts/gpu_par2_ab.py), one stream -> two branches: 16 tokens 8.66 -> 7.83
//     ms, 32: 9.17 -> 8.13, 128: 9.41 -> 8.82, 512: 26.75 -> 24.59, 1024: 49.3 -> 47.3, 2048: 104.9 -> 101.7.
//     (not where the mat-muls are passes of the k-quants' small-batch forms: they fill the chip and share one partial-sum scratch -- nor where a legacy K-share
//     mat-mul of each branch would write that scratch at once: fq_mm_par2_scratch_clash)
//     (round 6: lock-step passes of more than 32 sequences as well -- the same launches of ~50-100 us each, the decode attention of all sequences in the attention branch;
//     FALCON_HIP_PAR2_SEQS=0: those in stream order, as before)
//     (from 17 tokens for prompts -- 32 tokens 4.86 -> 4.70 ms, 20: 4.70 -> 4.62 --, from 33 sequences for lock-step passes, whose launches sit in the step's hipGraph:
//     32 per pass 4.78 -> 5.0 ms with it; profiles/r06zu_ab_par2_min_n.txt. FALCON_HIP_PAR2_MIN_N=n: both from n)
static int cols_out_width(const stage_block & b) {      // columns per output launch of the column form (Falcon-40B width: 2), 0: none
    return b.L.down.type == b.L.wo.type ? fq_gemv_out_cols_width(b.L.wo.type, b.L.down.K, b.L.wo.K) : 0;
}
static block_form block_form_of(const falcon_hip_context * c, const stage_block & b) {
    const fq_mm_switches & sw = fq_mm_sw();
    const layer_weights & L = b.L;
    const int N = b.N;
    if ((b.seq_stride || b.verify_limit) && N >= 2 && N <= cols_max_n(c->m) && c->fused_decode && !fq_reference_order() && !fq_attn_f64() &&
        L.qkv.type == L.up.type && cols_out_width(b) > 0 && !b.f16) return BLOCK_COLUMNS;
    const int par2_min_n = sw.par2_min_n ? sw.par2_min_n : (b.seq_stride ? 33 : 17);
    if (!b.verify_limit && !b.f16 && (!b.seq_stride || sw.par2_seqs) && N >= par2_min_n && N <= c->par2_max_n && !fq_prof_active() && !fq_ctx().dbg_stamps &&
        !fq_mm_par2_scratch_clash(fq_mm_mat_of(L.qkv), fq_mm_mat_of(L.wo), fq_mm_mat_of(L.up), fq_mm_mat_of(L.down), N, fq_ctx().n_cu, b.md, sw)) return BLOCK_TWO_STREAMS;
    return BLOCK_GENERIC;
}

// x = (Wdown a_ff + Wo a_att) + x, in stream order: the column form's output launches (cw_out > 0), the paired K-share / fused sum launch (5..16 columns, or
// passes of it), or Wo into its own matrix and Wdown with the residual epilogue
static void block_output(falcon_hip_context * c, const stage_block & b, int cw_out) {
    const layer_weights & L = b.L;
    const int64_t E = c->m->hp.n_embd;
    const int n_cu = fq_ctx().n_cu;
    hipStream_t st = b.st;
    if (cw_out > 0 && fq_col_passes(b.N, cw_out, false, "column output mat-vec", [&](const fq_col_window & cw) {
            const fq_gemv_out_cols_args go{ L.down, L.wo, cw.act(b.a_ff).base, cw.act(b.a_att).base, cw.dst(c->x, E), cw.dst(c->x, E), E, (int) cw.n };
            return fq_launch_gemv_out_cols(go, n_cu, st); })) return;
    const int min_cols = b.seq_stride ? 3 : 5;                             // (lock-step contexts: the k-quant small-batch forms from 3 sequences up)
    if (!b.f16 && fq_mul_mat_q_acts_out2(L.wo, b.a_att, L.down, b.a_ff, b.N, c->x, E, st, min_cols)) return;
    const fq_gemv_epi resid{ FQ_EPI_ADD2, fq_ctx().gelu_table, c->wo_out, c->x, E };          // x = (down + wo) + x, in place
    mm(b, L.wo, b.a_att, c->wo_out, E, epi_store(), st);
    mm(b, L.down, b.a_ff, c->x, E, resid, st);
}
// the generic form, in stream order: Wqkv [+ Wup in the same launch], attention, Wup + GELU, its image, the output
static void block_generic(falcon_hip_context * c, const stage_block & b, int cw_out = 0) {
    const layer_weights & L = b.L;
    const falcon_hip_hparams & hp = c->m->hp;
    const int64_t QKV = n_qkv(hp), FF = hp.n_ff;
    hipStream_t st = b.st;
    // Wqkv and Wup behind the same LayerNorm image (one-norm blocks): one launch of the small-batch mat-mul for both (5..32 columns)
    const bool pair_done = !b.f16 && b.a_qkv.base == b.a_up.base && b.a_qkv.type == b.a_up.type &&
                           fq_mul_mat_q_acts_pair(L.qkv, L.up, b.a_up, b.N, c->qkv, QKV, epi_store(), c->up, FF, epi_gelu(), st);
    if (!pair_done) mm(b, L.qkv, b.a_qkv, c->qkv, QKV, epi_store(), st);
    const bool ride = b.seq_stride && !fq_reference_order() && !fq_attn_f64() && fq_mm_sw().quant_rider && pair_done && (b.a_ff.type == FQ_Q8_0 || b.a_ff.type == FQ_Q8_1);
    block_attention(c, b, ride);
    bool ff_quantized = ride;
    // (k-quants, 5..16 columns or passes of them: GELU and Wdown's Q8_K image come out of the small-batch form's sum launch)
    if (!pair_done) {
        const int min_cols = b.seq_stride ? 3 : 5;
        if (!b.f16 && fq_mul_mat_q_acts_gelu_q8k(L.up, b.a_up, b.N, c->up, FF, b.a_ff, st, min_cols)) ff_quantized = true;
        else mm(b, L.up, b.a_up, c->up, FF, epi_gelu(), st);
    }
    if (!ff_quantized) fq_launch_quantize_act(c->up, FF, b.a_ff, st);
    block_output(c, b, cw_out);
}
// the column form (block_form_of). A first launch that refuses the shape (its LDS) leaves the block to the generic launches, which still try the column output launch
static void block_columns(falcon_hip_context * c, const stage_block & b) {
    const layer_weights & L = b.L;
    const falcon_hip_hparams & hp = c->m->hp;
    const int64_t QKV = n_qkv(hp), FF = hp.n_ff;
    const int n_cu = fq_ctx().n_cu, cw_out = cols_out_width(b);
    const bool quant_epi = (b.a_ff.type == FQ_Q8_0 || b.a_ff.type == FQ_Q8_1) && FF % 32 == 0;
    if (!fq_col_passes(b.N, 4, false, "column mat-vec", [&](const fq_col_window & cw) {
            fq_gemv_cols_args ga{};
            ga.nseg = 2; ga.ncols = (int) cw.n; ga.gelu_table = fq_ctx().gelu_table;
            ga.seg[0] = { L.qkv, cw.act(b.a_qkv).base, FQ_LNEPI_STORE, cw.dst(c->qkv, QKV), QKV, nullptr, 0, 0 };
            ga.seg[1] = { L.up, cw.act(b.a_up).base, quant_epi ? FQ_LNEPI_GELU_QUANT : FQ_LNEPI_GELU_STORE, cw.dst(c->up, FF), FF, cw.act(b.a_ff).base, b.a_ff.type, 0 };
            return fq_launch_gemv_cols(ga, n_cu, b.st); })) { block_generic(c, b, cw_out); return; }
    block_attention(c, b, false);
    if (!quant_epi) fq_launch_quantize_act(c->up, FF, b.a_ff, b.st);
    block_output(c, b, cw_out);
}
// the two-stream form (block_form_of): the MLP branch on the side stream. true: the residual sum was a launch of its own and carried the next block's LayerNorm(s)
static bool block_two_streams(falcon_hip_context * c, const stage_block & b) {
    const layer_weights & L = b.L;
    const falcon_hip_hparams & hp = c->m->hp;
    hip_context & hc = fq_ctx();
    const int64_t E = hp.n_embd, QKV = n_qkv(hp), FF = hp.n_ff;
    const int N = b.N;
    const size_t li = b.li;
    hipStream_t st = b.st;
    HIP_CHECK(hipEventRecord(c->ev_fork[li], st));
    HIP_CHECK(hipStreamWaitEvent(c->side, c->ev_fork[li], 0));
    mm(b, L.up, b.a_up, c->up, FF, epi_gelu(), c->side);
    fq_launch_quantize_act(c->up, FF, b.a_ff, c->side);
    mm(b, L.qkv, b.a_qkv, c->qkv, QKV, epi_store(), st);
    block_attention(c, b, false);
    // (round 6) Short prompts: neither branch waits for the other to carry the residual sum in an epilogue. Wdown -- the long launch of a short prompt (K = 4 n_embd,
    // 142 workgroups on 256 CUs at 128 tokens) -- follows Wup on the side stream and leaves its result in the (free again) f32 Wup matrix, Wo leaves its own, and
    // x = (down + wo) + x (libfalcon.cpp:2399-2400, the same additions in the same order) is a small launch behind the join.
    // Measured on MI355X, Falcon-7B Q4_0, epilogue form -> this (scripts/gpu_prompt_lengths.py, A/B/A/B on one box, profiles/r06zm_*): 40 tokens 6.80 -> 6.25 ms,
    // 64: 6.88 -> 6.40, 128: 8.17 -> 7.03 (18.2 k tok/s), 256: 14.3 -> 12.2, 512: 23.08 -> 23.00, 1024: 42.1 -> 41.6 -- but 384: 17.5 -> 18.2: Wdown's 426 workgroups
    // are 1.7 rounds of the chip there and the attention branch beside them only stretches the second. Hence: Wdown's launch at most 1.25 rounds or at least 2.
    // FALCON_HIP_PAR2_DOWN_FIRST=0: never (the epilogue form below), 2: always
    const int down_first = fq_mm_sw().par2_down_first;
    const int64_t down_wgs = fq_mm_gemm_wgs(fq_mm_mat_of(L.down), N, hc.n_cu, b.md, fq_mm_sw());      // (of the launch fq_launch_gemm will make: the same rules)
    if ((E & 3) == 0 && (down_first == 2 || (down_first == 1 && (4 * down_wgs <= 5 * (int64_t) hc.n_cu || down_wgs >= 2 * (int64_t) hc.n_cu)))) {
        mm(b, L.down, b.a_ff, c->up, E, epi_store(), c->side);
        HIP_CHECK(hipEventRecord(c->ev_join[li], c->side));
        mm(b, L.wo, b.a_att, c->wo_out, E, epi_store(), st);
        HIP_CHECK(hipStreamWaitEvent(st, c->ev_join[li], 0));
        fq_next_norm nn;
        if (next_norm(c, li + 1, N, nn)) { fq_launch_add2_ln(c->x, c->up, c->wo_out, E, N, nn, st); return true; }
        fq_launch_add2_inplace(c->x, c->up, c->wo_out, (int64_t) N * E, st);
        return false;
    }
    mm(b, L.wo, b.a_att, c->wo_out, E, epi_store(), st);
    HIP_CHECK(hipEventRecord(c->ev_attn[li], st));
    HIP_CHECK(hipStreamWaitEvent(c->side, c->ev_attn[li], 0));
    const fq_gemv_epi resid{ FQ_EPI_ADD2, hc.gelu_table, c->wo_out, c->x, E };          // x = (down + wo) + x, in place
    mm(b, L.down, b.a_ff, c->x, E, resid, c->side);
    HIP_CHECK(hipEventRecord(c->ev_join[li], c->side));
    HIP_CHECK(hipStreamWaitEvent(st, c->ev_join[li], 0));
    return false;
}

void fq_drv::launch_stage(falcon_hip_context * c, int N, int max_n_kv, hipStream_t st, int pos_stride, int verify_limit) {
    falcon_hip_model * m = c->m;
    const falcon_hip_hparams & hp = m->hp;
    const int64_t E = hp.n_embd, D = 64, HKV = hp.n_head_kv;

    if (m->first_stage()) fq_launch_dequant_rows(m->tok_emb, c->tokens_dev, N, c->x, st);    // ggml_get_rows, libfalcon.cpp:2120

    const int64_t seq_stride = c->n_seq > 0 ? (int64_t) c->n_ctx * HKV * D : 0;             // lock-step sequences: one KV cache per row
    const int64_t n_caches = c->n_seq > 0 ? c->n_seq : 1;
    if (c->n_seq > 0 && N != c->n_seq) { fprintf(stderr, "falcon-hip: a context of %d lock-step sequences evaluates %d rows per step, not %d\n", c->n_seq, c->n_seq, N); exit(1); }
    const int * seq_pos = pos_stride ? c->pos_dev : c->n_past_dev;                         // what the lock-step attention launches read
    if (pos_stride && !seq_stride) { fprintf(stderr, "falcon-hip: per-row positions need a lock-step context\n"); exit(1); }
    // the fused kernels are instantiated per weight format: a model that mixes formats inside a block (e.g. the reference's
    // Q4_K_M for Falcon-7B: only the 18176-wide Wdown can hold 256-element super-blocks) takes the op list
    if (N == 1 && stage_fused(c)) { launch_stage_token(c, max_n_kv, st); return; }
    // LayerNorm of x + the image its consumer takes. An F16 consumer (ggml_compute_forward_mul_mat_f16_f32's INIT phase, ggml.c:11176-11196): the f32 rows of
    // ggml_norm, mul, add, then their fp16 image (kernels_f16.hip)
    auto ln_image = [&](const float * w, const float * b, const fq_act & a, float * y = nullptr) {
        if (a.type == FQ_F16) { fq_launch_layer_norm(c->x, E, N, w, b, c->ln, st); fq_launch_quantize_act(c->ln, E, a, st); }
        else fq_launch_layer_norm_quant(c->x, E, N, w, b, y, a, st);                         // (y: the f32 rows, needed by the embeddings only)
    };
    bool ln_done = false;                                   // this block's LayerNorm image(s) came out of the previous block's residual-sum launch
    const fq_mm_mode md = fq_mm_mode_now();
    for (size_t li = 0; li < m->layers.size(); ++li) {
        const layer_weights & L = m->layers[li];
        if (c->keep_hidden) HIP_CHECK(hipMemcpyAsync(c->hidden_dev + li * (size_t) N * E, c->x, (size_t) N * E * 4, hipMemcpyDeviceToDevice, st));
        const fq_act a_up = act_for(c->buf_e, L.up, N);
        fq_act a_qkv = a_up;
        if (hp.two_norms) {                                                              // ln_mlp and ln_attn: one launch when both images are of one type
            a_qkv = act_for(c->buf_e2, L.qkv, N);
            if (ln_done) {
            } else if (a_up.type == FQ_F16 || a_qkv.type == FQ_F16 || !fq_launch_layer_norm_quant2(c->x, E, N, L.ln_w, L.ln_b, a_up, L.ln2_w, L.ln2_b, a_qkv, st)) {
                ln_image(L.ln_w, L.ln_b, a_up);
                ln_image(L.ln2_w, L.ln2_b, a_qkv);
            }
        } else if (!ln_done) ln_image(L.ln_w, L.ln_b, a_up);
        ln_done = false;
        if (hp.two_norms) {
        } else if (act_for(c->buf_e2, L.qkv, N).type != a_up.type) {                     // same norm, the other activation family
            a_qkv = act_for(c->buf_e2, L.qkv, N);
            ln_image(L.ln_w, L.ln_b, a_qkv);
        }
        const size_t cache_off = li * (size_t) n_caches * c->n_ctx * HKV * D;
        const stage_block b{ L, li, layer_has_f16(L), c->k_cache + cache_off, c->v_cache + cache_off, a_qkv, a_up, act_for(c->buf_att, L.wo, N), act_for(c->buf_ff, L.down, N),
                             N, max_n_kv, seq_pos, seq_stride, pos_stride, verify_limit, st, md };
        switch (block_form_of(c, b)) {
            case BLOCK_COLUMNS:     block_columns(c, b); break;
            case BLOCK_TWO_STREAMS: ln_done = block_two_streams(c, b); break;
            case BLOCK_GENERIC:     block_generic(c, b); break;
        }
    }
    if (c->keep_hidden) {
        HIP_CHECK(hipMemcpyAsync(c->hidden_dev + m->layers.size() * (size_t) N * E, c->x, (size_t) N * E * 4, hipMemcpyDeviceToDevice, st));
        c->hidden_tokens = N;
    }
    if (m->last_stage()) {
        const fq_act a_head = act_for(c->buf_e, m->lm_head, N);
        if (!ln_done) ln_image(m->out_norm_w, m->out_norm_b, a_head, c->emb_mode ? c->emb_rows : nullptr);
        if (c->emb_mode) {
            // the ln_f rows: out of the launch above (an F16 head's are in c->ln), or -- the last block's residual-sum launch made the head's image -- by one plain LayerNorm
            const float * rows = !ln_done && a_head.type == FQ_F16 ? c->ln : c->emb_rows;
            if (ln_done) fq_launch_layer_norm(c->x, E, N, m->out_norm_w, m->out_norm_b, c->emb_rows, st);
            HIP_CHECK(hipMemcpyAsync(c->emb, rows + (size_t)(N - 1) * E, (size_t) E * 4, hipMemcpyDeviceToDevice, st));      // libfalcon.cpp:2551-2557: the last token's
            if (c->emb_mode & FALCON_HIP_EMBED_POOL) fq_launch_embed_pool_accum(rows, N, (int) E, c->pool_acc, c->pool_count, st);
            if (c->emb_no_head) return;
        }
        // (2..cols_max_n rows of a lock-step context or a verify pass: the column mat-vec launch, as the blocks)
        if ((seq_stride || verify_limit) && N >= 2 && N <= cols_max_n(m) && c->fused_decode && !fq_reference_order() && m->lm_head.type != FQ_F16 &&
            fq_col_passes(N, 4, false, "column mat-vec (lm_head)", [&](const fq_col_window & cw) {
                fq_gemv_cols_args ga{};
                ga.nseg = 1; ga.ncols = (int) cw.n; ga.gelu_table = fq_ctx().gelu_table;
                ga.seg[0] = { m->lm_head, cw.act(a_head).base, FQ_LNEPI_STORE, cw.dst(c->logits_dev, hp.n_vocab), hp.n_vocab, nullptr, 0, 0 };
                return fq_launch_gemv_cols(ga, fq_ctx().n_cu, st); })) return;
        if (seq_stride) fq_mul_mat_q_acts_from3(m->lm_head, a_head, N, c->logits_dev, hp.n_vocab, epi_store(), st);      // all N rows, libfalcon.cpp:2440
        else fq_mul_mat_q_acts(m->lm_head, a_head, N, c->logits_dev, hp.n_vocab, epi_store(), st);
    }
}
