// kernels_sample_row.h -- the body of one sampled row, included (not called) by kernels_sample.hip's two users of it: k_sample_rows, one row per workgroup,
// and sk_row, which k_verify_rows runs over the rows of a draft-and-verify pass. Text, not a function, for k_sample_rows' sake: called as an inlined
// device function the same body compiled to other register counts in the kernel's TEXT instantiations (NOTEBOOK, the section on draft-and-verify decode); included,
// the kernel is the token stream it always was. The including scope provides: EXT, TEXT, MASK, the kernel's arguments but logits and stride, and
//   gram            MASK: the rows' grammar bindings (fq_grammar.h's fq_grammar_row, trans == nullptr: this row is unconstrained); otherwise not read
//   const int row   the sampler row whose state draws and advances
//   const int tid   threadIdx.x
//   SK_ROW_X        the logits row the draw is made from
//   SK_ROW_ENDED    what to do (return ...) when the row's stops had ended it before the launch: nothing of the row has moved
//   GUIDE, sk_guide GUIDE: the row's guide row (ggml_hip_sampler_set_guidance; -1: none). The drawing lane writes for it what it writes for the row, where and
//                   when it does so for the row: the skip word, the output slot and step counter, the next token and position. Otherwise false and -1
    __shared__ uint32_t flag[FQ_SK_MAX_VOCAB / 32];
    __shared__ int hkey[FQ_SK_HASH], hcnt[FQ_SK_HASH];
    __shared__ uint64_t keys[FQ_SK_SMALL_K];
    __shared__ uint32_t mt[FQ_MT_N + 1];
    __shared__ int hist[256];
    __shared__ int b_id[FQ_SAMPLE_MAX_BIAS];
    __shared__ float b_val[FQ_SAMPLE_MAX_BIAS];
    __shared__ float red_v[FQ_SK_THREADS / 64];
    __shared__ int red_i[FQ_SK_THREADS / 64];
    __shared__ uint64_t sh_prefix;
    __shared__ int sh_rem, sh_done, sh_cnt, sh_tok;
    __shared__ uint32_t t_cfgw[TEXT ? FQ_SK_TEXT_CFG_W : 1], t_stw[TEXT ? FQ_SK_TEXT_ST_W : 1];      // the row's strings; its ring and byte count as the launch found them
    __shared__ uint8_t t_win[TEXT ? FQ_STOPT_MAX_LEN + 64 : 1];                                     // the drawn text's last 32 bytes before a chunk of the token, then the chunk

    const bool stops = stop_cfg && stop_cfg[row].on;
    if (stop_cfg) {                                         // (block-uniform; only this workgroup touches the row's words)
        const bool ended = stops && fq_stop_finished(&stop_state[row]);
        if (tid == 0) {
            stop_skip[row] = ended ? 1 : 0;
            if constexpr (GUIDE) { if (sk_guide >= 0) stop_skip[sk_guide] = ended ? 1 : 0; }
        }
        if (ended) SK_ROW_ENDED;
    }
    if constexpr (TEXT) {                                   // (visible behind the barriers every path below passes before its draw)
        if (stops && tid < FQ_SK_TEXT_CFG_W) t_cfgw[tid] = ((const uint32_t *) &text.cfg[row])[tid];
        if (stops && tid >= FQ_SK_TEXT_ST_T0 && tid < FQ_SK_TEXT_ST_T0 + FQ_SK_TEXT_ST_W) t_stw[tid - FQ_SK_TEXT_ST_T0] = ((const uint32_t *) &text.state[row])[tid - FQ_SK_TEXT_ST_T0];
    }
    const fq_sample_row & P = rows[row];
    const float temp = P.temp, penalty = P.penalty, alpha_f = P.alpha_f, alpha_p = P.alpha_p;
    const int W = P.W, n_bias = P.n_bias;
    const float * x = SK_ROW_X;
    int32_t * rg = ring + (int64_t) row * ring_cap;
    // MASK: the index row of the state the launch found the row in, as 32-bit words (bit t % 32 of word t / 32: the 64-bit index words are little-endian);
    // it stays in HBM / L2 through the passes -- adjacent lanes read the same word
    const uint32_t * g_allow = nullptr;
    if constexpr (MASK) { if (gram[row].trans) g_allow = (const uint32_t *)(gram[row].allow + (int64_t) gram[row].state * gram[row].n_words); }

    for (int i = tid; i < (n + 31) / 32; i += FQ_SK_THREADS) flag[i] = 0;
    for (int i = tid; i < FQ_SK_HASH; i += FQ_SK_THREADS) { hkey[i] = -1; hcnt[i] = 0; }
    if (tid < n_bias) { b_id[tid] = P.bias_id[tid]; b_val[tid] = P.bias[tid]; }
    __syncthreads();
    for (int j = tid; j < W; j += FQ_SK_THREADS) {
        const int id = rg[j];
        atomicOr(&flag[id >> 5], 1u << (id & 31));
        for (int s = sk_hash(id);; s = (s + 1) & (FQ_SK_HASH - 1)) {
            const int o = atomicCAS(&hkey[s], -1, id);
            if (o == -1 || o == id) { atomicAdd(&hcnt[s], 1); break; }
        }
    }
    if (tid < n_bias) atomicOr(&flag[b_id[tid] >> 5], 1u << (b_id[tid] & 31));
    __syncthreads();

    // the candidate's logit after bias and penalties (falcon_main.cpp:898-956)
    auto pen = [&](int i, float v) -> float {
        if ((flag[i >> 5] >> (i & 31)) & 1u) {
            bool bon = false; float b = 0.0f;
            for (int j = 0; j < n_bias; ++j) if (b_id[j] == i) { bon = true; b = b_val[j]; }
            int cnt = 0;
            for (int s = sk_hash(i);; s = (s + 1) & (FQ_SK_HASH - 1)) {
                const int k = hkey[s];
                if (k == i) { cnt = hcnt[s]; break; }
                if (k == -1) break;
            }
            v = fq_penalize(v, bon, b, cnt, penalty, alpha_f, alpha_p);
        }
        return v;
    };
    // f(i, penalised logit i) over this thread's share of the row, FQ_SK_UNROLL loads in flight (one load per iteration is a chain
    // of round trips: ~20 us per pass over 65024 logits)
    auto pass = [&](auto f) {
        for (int i0 = tid; i0 < n; i0 += FQ_SK_UNROLL * FQ_SK_THREADS) {
            float r[FQ_SK_UNROLL];
            uint32_t aw[MASK ? FQ_SK_UNROLL : 1];           // MASK: the index words of the same ids, in flight with the logits (read where they are used, each is a round trip of its own: +34 us a step)
#pragma unroll
            for (int u = 0; u < FQ_SK_UNROLL; ++u) {
                const int i = i0 + u * FQ_SK_THREADS;
                r[u] = x[i < n ? i : n - 1];
                if constexpr (MASK) aw[u] = g_allow ? g_allow[(i < n ? i : n - 1) >> 5] : 0xffffffffu;
            }
#pragma unroll
            for (int u = 0; u < FQ_SK_UNROLL; ++u) {
                const int i = i0 + u * FQ_SK_THREADS;
                if constexpr (MASK) {                       // a forbidden candidate: -inf behind bias and penalties (fq_grammar.h)
                    if (i < n) { const float v = pen(i, r[u]); f(i, (aw[u] >> (i & 31)) & 1u ? v : -INFINITY); }
                } else if (i < n) f(i, pen(i, r[u]));
            }
        }
    };

    if (temp <= 0.0f) {
        // llama_sample_token_greedy: the first maximum in id order
        float best = -INFINITY; int idx = 0x7FFFFFFF;
        pass([&](int i, float v) { if (v > best || (v == best && i < idx)) { best = v; idx = i; } });
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(best, o); const int oi = __shfl_xor(idx, o);
            if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
        }
        if ((tid & 63) == 0) { red_v[tid >> 6] = best; red_i[tid >> 6] = idx; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < FQ_SK_THREADS / 64; ++w) if (red_v[w] > best || (red_v[w] == best && red_i[w] < idx)) { best = red_v[w]; idx = red_i[w]; }
            sh_tok = idx < n ? idx : 0;                   // (a row of NaN: no maximum)
        }
    } else {
        int k = P.top_k <= 0 ? n : P.top_k;                 // llama_sample_top_k with min_keep 1
        k = k < 1 ? 1 : (k > n ? n : k);
        fq_sample_ext X = { 1.0f, 1.0f, 0.0f, 0.0f, 0 };
        if constexpr (EXT) X = ext[row];
        const bool chain = EXT && X.mirostat == 0 && (!(X.tfs_z >= 1.0f) || !(X.typical_p >= 1.0f));     // (set_row_ext: then 1 <= top_k <= FQ_SK_SMALL_K)
        for (int i = tid; i <= FQ_MT_N; i += FQ_SK_THREADS) mt[i] = mtg[(int64_t) row * (FQ_MT_N + 1) + i];
        if (k <= FQ_SK_SMALL_K && !(EXT && X.mirostat != 0)) {
            // radix select of the k-th largest key, 8 bits at a time; stops as soon as the selected bucket is taken whole
            uint64_t prefix = 0; int rem = k, s_exit = 0;
            for (int shift = 56; shift >= 0; shift -= 8) {
                for (int i = tid; i < 256; i += FQ_SK_THREADS) hist[i] = 0;
                __syncthreads();
                pass([&](int i, float v) {
                    const uint64_t K = fq_sort_key(v, i);
                    if (shift == 56 || (K >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(K >> shift) & 255], 1);
                });
                __syncthreads();
                if (tid == 0) {
                    int r = rem, d = 255;
                    while (hist[d] < r) { r -= hist[d]; --d; }
                    sh_prefix = prefix | ((uint64_t) d << shift); sh_rem = r; sh_done = hist[d] == r;
                }
                __syncthreads();
                prefix = sh_prefix; rem = sh_rem; s_exit = shift;
                if (sh_done) break;
            }
            if (tid == 0) sh_cnt = 0;
            __syncthreads();
            pass([&](int i, float v) {
                const uint64_t K = fq_sort_key(v, i);
                if ((K >> s_exit) >= (prefix >> s_exit)) { const int slot = atomicAdd(&sh_cnt, 1); if (slot < FQ_SK_SMALL_K) keys[slot] = K; }      // (exactly k: the keys are distinct)
            });
            int kp = 1;
            while (kp < k) kp <<= 1;
            for (int i = k + tid; i < kp; i += FQ_SK_THREADS) keys[i] = 0;
            __syncthreads();
            sk_bitonic_desc(keys, kp, tid);
            if (!chain) {
                if (tid == 0) {
                    sk_lsrc src{ keys };
                    int mti = (int) mt[FQ_MT_N];
                    const int p = fq_sample_tail(src, k, P.top_p, temp, mt, &mti);
                    mt[FQ_MT_N] = (uint32_t) mti;
                    sh_tok = fq_key_id(keys[p]);
                }
            } else if constexpr (EXT) {
                // top-k, tail-free, typical, top-p, temperature, draw (fq_sample_chain.h) on the k <= FQ_CHAIN_MAX sorted survivors
                static_assert(FQ_CHAIN_MAX == FQ_SK_SMALL_K, "tail-free and typical take the LDS form's survivors");
                __shared__ float cp[FQ_CHAIN_MAX];          // probabilities, then scratch of the stage at hand
                __shared__ uint64_t tk[FQ_CHAIN_MAX];       // typical's keys: (shifted score, position in logit order)
                __shared__ int sh_n;
                const bool typ = !(X.typical_p >= 1.0f);
                sk_lsrc src{ keys };
                if (tid == 0) {
                    const int n1 = fq_tail_free(src, k, X.tfs_z, cp);
                    if (typ) fq_typical_scores(src, n1, cp, tk);
                    sh_n = n1;
                }
                __syncthreads();
                const int n1 = sh_n;
                if (typ) {                                  // ascending by key == descending by its complement (never 0: a score's sign bit is clear)
                    int np2 = 1;
                    while (np2 < n1) np2 <<= 1;
                    for (int i = tid; i < np2; i += FQ_SK_THREADS) tk[i] = i < n1 ? ~tk[i] : 0;
                    __syncthreads();
                    sk_bitonic_desc(tk, np2, tid);
                    for (int i = tid; i < n1; i += FQ_SK_THREADS) tk[i] = ~tk[i];
                    __syncthreads();
                }
                if (tid == 0) {
                    int mti = (int) mt[FQ_MT_N], at;
                    if (typ) {                              // the survivors stay in score order for everything behind typical
                        const int n2 = fq_typical_cut(cp, tk, n1, X.typical_p);
                        auto val2 = [&](int i) { return fq_key_val(keys[fq_typical_pos(tk[i])]); };
                        at = fq_typical_pos(tk[fq_chain_tail(val2, n2, P.top_p, temp, cp, mt, &mti)]);
                    } else
                        at = fq_chain_tail(src, n1, P.top_p, temp, cp, mt, &mti);
                    mt[FQ_MT_N] = (uint32_t) mti;
                    sh_tok = fq_key_id(keys[at]);
                }
            }
        } else {
            uint64_t * sk = sortg + (int64_t) row * np;
            pass([&](int i, float v) { sk[i] = fq_sort_key(v, i); });
            for (int i = n + tid; i < np; i += FQ_SK_THREADS) sk[i] = 0;
            __syncthreads();
            sk_bitonic_desc(sk, np, tid);
            if (tid == 0) {
                sk_gsrc src{ sk, keys, -FQ_SK_GBUF, n };
                int mti = (int) mt[FQ_MT_N];
                int p;
                if (EXT && X.mirostat != 0) {               // temperature, mirostat 1 / 2 on the whole sorted row; N = the sampler's n_vocab
                    float mu = mug[row];
                    p = fq_mirostat(src, n, X.mirostat, temp, X.tau, X.eta, n, &mu, mt, &mti, nullptr, nullptr);
                    mug[row] = mu;
                } else
                    p = fq_sample_tail(src, k, P.top_p, temp, mt, &mti);
                mt[FQ_MT_N] = (uint32_t) mti;
                sh_tok = fq_key_id(sk[p]);
            }
        }
        __syncthreads();
        for (int i = tid; i <= FQ_MT_N; i += FQ_SK_THREADS) mtg[(int64_t) row * (FQ_MT_N + 1) + i] = mt[i];
    }
    if (tid == 0) {
        const int t = sh_tok;
        if (W > 0) { const int h = head[row]; rg[h] = t; head[row] = h + 1 == W ? 0 : h + 1; }
        if (stops) fq_stop_draw(&stop_cfg[row], &stop_state[row], t);
        if constexpr (MASK) {                               // the row's state moves with every draw, also the one that ends the row
            fq_grammar_row & G = gram[row];
            if (G.trans) G.state = fq_grammar_advance(G.trans, G.state, t, G.eos_id, G.pool, G.offs);
        }
        if (out) { const int s = steps[row]; out[(int64_t) s * out_stride + row] = t; steps[row] = s + 1; }
        if constexpr (GUIDE) { if (out && sk_guide >= 0) { const int s = steps[sk_guide]; out[(int64_t) s * out_stride + sk_guide] = t; steps[sk_guide] = s + 1; } }
        if (drawn) drawn[row] = t;
    }
    if constexpr (TEXT) {
        // fq_stop_text.h on the wave of the drawing lane: lane j takes byte c0 + j of the token. t_win[32 + j] is that byte and t_win[0 .. 32) the 32 bytes of
        // the drawn text before the chunk (the ring at first, then the chunk before), so "i places back" is one LDS read whichever token the byte came from.
        const fq_stopt_cfg & tc = *(const fq_stopt_cfg *) t_cfgw;
        if (tid < 64 && stops && tc.n > 0) {
            const fq_stopt_state & ts = *(const fq_stopt_state *) t_stw;
            const int lane = tid;
            const int t = __shfl(sh_tok, 0);                // (lane 0 wrote it, or read it behind a barrier)
            const int n0 = ts.n_bytes;
            const int o0 = text.offs[t], L = text.offs[t + 1] - o0;
            const uint8_t * b = text.pool + o0;
            if (lane < FQ_STOPT_MAX_LEN) t_win[lane] = ts.ring[(n0 + lane) & (FQ_STOPT_MAX_LEN - 1)];
            int best = 0x7FFFFFFF, c0 = 0;                  // the smallest j * FQ_STOPT_MAX + k
            for (;; c0 += 64) {
                const int p = c0 + lane;
                if (p < L) t_win[FQ_STOPT_MAX_LEN + lane] = b[p];
                sk_wave_sync();
                int key = 0x7FFFFFFF;
                if (p < L) {
                    const uint8_t * at = t_win + FQ_STOPT_MAX_LEN + lane;
                    const int k = fq_stopt_match_at(&tc, (int64_t) n0 + p + 1, [&](int i) { return at[-i]; });
                    if (k >= 0) key = p * FQ_STOPT_MAX + k;
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) { const int ok = __shfl_xor(key, o); key = ok < key ? ok : key; }
                best = key < best ? key : best;
                if (c0 + 64 >= L) break;
                sk_wave_sync();                             // (every lane has read the window: its last 32 bytes become its first)
                if (lane < FQ_STOPT_MAX_LEN) t_win[lane] = t_win[64 + lane];
                sk_wave_sync();                             // (... before the next chunk lands on them)
            }
            if (L > 0) {                                    // the ring: the text's last 32 bytes, t_win[cnt .. cnt + 32) behind a last chunk of cnt bytes
                const int cnt = L - c0;
                if (lane < FQ_STOPT_MAX_LEN) text.state[row].ring[(n0 + L + lane) & (FQ_STOPT_MAX_LEN - 1)] = t_win[cnt + lane];
            }
            if (lane == 0) {
                text.state[row].n_bytes = fq_stopt_count(n0, L);
                const bool hit = best != 0x7FFFFFFF;
                fq_stopt_end(&tc, &text.state[row], &stop_state[row], stop_state[row].reason, hit ? best / FQ_STOPT_MAX : 0, hit ? best % FQ_STOPT_MAX : -1, L);
            }
        }
    }
    // the row's next token and position move last, behind every rule that may end the row (this thread ran them all): a row
    // whose draw fills its cache ends here if nothing else ended it (fq_stop_context) and keeps both, so that riding on frozen
    // it evaluates the same token at the same position -- never at ctx_limit, the first row of the next slot
    if (tid == 0) {
        const int p = pos ? pos[row] : 0;
        if (!(pos && stops && fq_stop_context(&stop_state[row], p, ctx_limit))) {
            token[row] = sh_tok;
            if (pos) pos[row] = p + 1;
            if constexpr (GUIDE) { if (sk_guide >= 0) { token[sk_guide] = sh_tok; if (pos) pos[sk_guide] = pos[sk_guide] + 1; } }
        }
    }
