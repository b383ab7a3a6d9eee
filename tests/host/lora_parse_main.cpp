// lora_parse_main.cpp -- TEST INFRASTRUCTURE: a stand-alone host program over csrc/fq_lora.h (tests/test_lora_cpu.py compiles it, with
// -fsanitize=address,undefined where the compiler has the runtimes): parses every adapter file it is given from a heap buffer of exactly the file's size, so
// that a read past the end is a reported error and not a quiet one, and reads every byte a successful parse points at.
//   lora_parse_main N_VOCAB N_EMBD N_HEAD N_HEAD_KV N_LAYER N_FF  FILE CODE [FILE CODE ...]      exit 0 when every parse returned its expected code
#include "fq_lora.h"
#include <cstdio>
#include <cstdlib>

int main(int argc, char ** argv) {
    if (argc < 9 || (argc - 7) % 2) { fprintf(stderr, "usage: %s N_VOCAB N_EMBD N_HEAD N_HEAD_KV N_LAYER N_FF FILE CODE [FILE CODE ...]\n", argv[0]); return 2; }
    const fq_lora_hparams hp{ atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]) };
    int bad = 0;
    for (int a = 7; a + 1 < argc; a += 2) {
        const int want = atoi(argv[a + 1]);
        char msg[1400];
        std::vector<uint8_t> file;
        fq_lora_view v;
        v.r = -77; v.alpha = -78;
        int rc = fq_lora_read(argv[a], hp, &file, &v, msg, sizeof msg);
        if (rc != FQ_LORA_E_IO) {                                      // again from a buffer of exactly the file's size
            const size_t n = file.size();
            uint8_t * p = (uint8_t *) malloc(n ? n : 1);
            memcpy(p, file.data(), n);
            fq_lora_view w;
            w.r = -77; w.alpha = -78;
            const int rc2 = fq_lora_parse(p, n, hp, &w, msg, sizeof msg);
            if (rc2 != rc) { printf("%s: the two parses disagree (%d, %d)\n", argv[a], rc, rc2); ++bad; }
            if (rc2 != FQ_LORA_OK && (w.r != -77 || w.alpha != -78 || !w.pairs.empty())) { printf("%s: a refusal wrote its output\n", argv[a]); ++bad; }
            if (rc2 == FQ_LORA_OK) {
                unsigned sum = 0;
                for (const fq_lora_pair & pr : w.pairs)
                    for (const fq_lora_half * h : { &pr.a, &pr.b }) {
                        if (h->offset > n || h->bytes > n - h->offset) { printf("%s: %s points outside the file\n", argv[a], pr.name.c_str()); ++bad; continue; }
                        for (size_t i = 0; i < h->bytes; ++i) sum += p[h->offset + i];
                    }
                printf("  (r %d, alpha %d, %zu pairs, checksum %u)\n", w.r, w.alpha, w.pairs.size(), sum);
            }
            free(p);
        }
        printf("%s: code %d (expected %d)%s%s\n", argv[a], rc, want, rc ? ": " : "", rc ? msg : "");
        bad += rc != want;
    }
    return bad ? 1 : 0;
}
