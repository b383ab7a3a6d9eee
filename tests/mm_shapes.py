"""The (K, M, N) shapes the op-level GPU mat-mul tests run (tests/test_gpu_mul_mat.py, tests/test_gpu_op_contract.py), in one place: the GPU tests
parametrize from these lists and tests/test_mm_coverage_cpu.py computes, on the CPU, the launch key (csrc/fq_mm_forms.h fq_mm_launch_key) of every one of
them and holds the set against the keys the Falcon-7B / 40B / 180B matrices take. A shape deleted here leaves both at once.

No GPU, no oracle in here. A case is (type, K, M, N, mode); mode "default", "seq" (ggml_hip_gemm_sequential), "ref1" / "ref2" (ggml_hip_reference_order) or
"cfg<c>" (FQ_GEMM_CFG=c)."""
Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q2_K, Q3_K, Q4_K, Q5_K, Q6_K = 2, 3, 6, 7, 8, 10, 11, 12, 13, 14
LEGACY = (Q4_0, Q4_1, Q5_0, Q5_1, Q8_0)
KQUANTS = (Q2_K, Q3_K, Q4_K, Q5_K, Q6_K)
WEIGHT_TYPES = LEGACY + KQUANTS
BLCK = {t: 32 for t in LEGACY}
BLCK.update({t: 256 for t in KQUANTS})

# ---------------------------------------------------------------------------------------------- tests/test_gpu_mul_mat.py
MUL_MAT_KM = [(512, 37), (4544, 70), (8192, 129), (18176, 33)]
MUL_MAT_N = [1, 2, 3, 5]
PREFILL_GEMM = [(512, 37, 9), (4544, 200, 33), (8192, 129, 128), (1024, 300, 257), (18176, 70, 40),
                (4544, 200, 16), (18176, 70, 12), (8192, 129, 5), (4544, 100, 7), (4672, 33, 13),      # (N <= 16: the streaming form, kernels_gemm_skinny.hip)
                (4544, 200, 17), (8192, 129, 32), (18176, 70, 29),                              # (17..32: two passes of it)
                (4736, 70, 40), (4992, 70, 130), (4864, 40, 64)]                                # (37 / 39 / 38 K stages: the tails of the two-stages-per-barrier loop)
Q4K_SMALL_BATCH = [(2048, 64, 7), (2560, 48, 16), (8192, 144, 5), (10240, 32, 13), (16384, 16, 16), (8192, 144, 29), (4096, 64, 77), (4096, 32, 100), (2048, 20480, 6),
                   (10240, 20480, 5)]
Q4K_SMALL_BATCH_TYPES = [Q4_K, Q5_K, Q2_K, Q3_K, Q6_K]
ROWS64 = [(512, 37, 9), (4544, 200, 33), (8192, 129, 130), (1024, 300, 257)]        # test_prefill_gemm_64_row_workgroups, FQ_GEMM_CFG 6 and (legacy) 7

# ---------------------------------------------------------------------------------------------- tests/test_gpu_op_contract.py
MAT_VEC = (512, 37, [1, 2, 3, 4])
LEGACY_FORMS = [
    (512, 37, 5),        # k_gemm_skinny_res: the columns resident in LDS, one 32-row pair, 16 blocks
    (4544, 200, 16),     # k_gemm_skinny_res: seven row pairs (the last partial), a full 16 columns, a partial last stage (142 blocks)
    (6144, 40, 9),       # k_gemm_skinny: the streaming form (192 blocks: the columns no longer fit LDS, fewer than the K-share form's 256)
    (8192, 129, 5),      # k_gemm_skinny_ks + k_skinny_sum4: one K share per workgroup (256 blocks)
    (4544, 200, 17),     # 17..32 columns: two passes of the resident form (16 + 1 columns; add1 += 16 * ld_add)
    (8192, 129, 29),     # ... of the K-share form (16 + 13)
    (512, 37, 33),       # k_gemm_q<4, 2>: the tile GEMM with 64-token tiles (33..64 columns)
    (512, 37, 70),       # k_gemm_q<4, 4>: 128-token tiles
]
LEGACY_TILE_CFGS, KQUANT_TILE_CFGS = [1, 3, 6, 7], [1, 3, 6]
TILE_INSTANTIATION = (512, 70, 40)       # under each of those FQ_GEMM_CFG
SINGLE_SUM_TILE = (512, 37, 130)         # FQ_GEMM_CFG=0, legacy
SEQ16 = (512, 37, 40)                    # ggml_hip_gemm_sequential, legacy
KQUANT_FORMS = [
    (512, 37, 9),        # k_gemm_q<4, 1>: the tile GEMM (2 super-blocks: fewer than the small-batch forms' 8)
    (2048, 64, 7),       # k_gemm_skinny_q4k / _q2k / _q6k + k_skinny_sum4: the small-batch form, 8 super-blocks, four 16-row tiles
    (2560, 48, 16),      # ... a partial last group of super-blocks (10), 16 columns
    (2048, 37, 7),       # M % 16 != 0: the small-batch form declines, the tile GEMM takes 7 columns
    (8192, 144, 29),     # two passes of 16 columns (16 + 13), 32 super-blocks: one segment (Q4_K / Q5_K) or two (Q2_K / Q3_K / Q6_K)
    (4096, 32, 80),      # five passes: the last width of Q4_K / Q5_K / Q6_K's small-batch form ..
    (4096, 32, 81),      # .. and the first of their tile GEMM (Q2_K / Q3_K: six passes)
    (4096, 32, 112),     # seven passes: the last width of Q2_K / Q3_K's ..
    (4096, 32, 113),     # .. and every k-quant on the tile GEMM
]
ORDER_SHAPES = {"legacy": [(512, 37, 3), (512, 37, 5), (512, 37, 33)], "kquant": [(512, 37, 3), (2048, 64, 7), (512, 37, 9)]}
ORDER_MODES = ["seq", "ref1", "ref2"]
FEW_M, FEW_N = [1, 3, 33], [1, 3, 5, 17, 40]
FEW_K_LEGACY, FEW_K_KQUANTS = [32, 64, 96, 160], [256, 512, 768]

# ---- the small-batch forms only model-sized matrices reach (test_legacy_model_forms): the smallest shapes that land, for all five legacy formats on 256 CUs,
# in each launch key the Falcon-7B / 40B / 180B matrices take at 5..32 columns. Row counts are no multiples of 32 on purpose. (K, M, N, mode, formats)
MODEL_FORMS_LEGACY = [
    (512, 32741, 5, "default", LEGACY),            # k_gemm_skinny_res<T, 2, 3>: two K shares, persistent workgroups looping over 1024 row pairs
    (512, 32741, 17, "default", LEGACY),           # .. two passes
    (4544, 32741, 5, "default", LEGACY),           # .. at Falcon-7B's K: NBW 3 (Q4_0, Q4_1), NBW 2 (Q5_0, Q5_1); Q8_0: k_gemm_skinny<T, 2>
    (6144, 32741, 5, "default", LEGACY),           # k_gemm_skinny<T, 2>: the per-stage form at two K shares
    (6144, 32741, 17, "default", (Q4_0, Q5_1)),    # .. two passes (3.4 G multiply-adds: two formats)
    (6144, 40, 17, "default", LEGACY),             # k_gemm_skinny<T, 4>, two passes
    (512, 8229, 9, "default", LEGACY),             # the resident form, 258 row pairs on 256 workgroups: S = 4, NBW 3
    (512, 8229, 20, "default", LEGACY),            # .. two passes
    (4544, 8229, 16, "default", LEGACY),           # .. NBW 3 and 2, 16 columns
    (512, 8229, 9, "seq", LEGACY),                 # the same three with one K share (S = 1)
    (512, 8229, 20, "seq", LEGACY),
    (4544, 8229, 16, "seq", LEGACY),
    (8192, 1040, 5, "default", LEGACY),            # k_gemm_skinny_ks: T = 2 tiles per workgroup
    (8192, 4544, 7, "default", LEGACY),            # .. T = 5, NBW 3
    (18176, 4544, 12, "default", LEGACY),          # .. T = 5 at 568 blocks: NBW 2 for Q5_0, Q5_1, Q8_0
    (8192, 8192, 16, "default", LEGACY),           # .. T = 8, every row block has its slot
    (8192, 9216, 5, "default", LEGACY),            # .. T = 8, 72 row blocks on 64 slots: the walk
    (8192, 9216, 29, "default", LEGACY),           # .. two passes
    (8192, 32736, 16, "default", (Q4_0,)),         # .. the K-share form's largest M: 256 row blocks on 64 slots
]


def model_forms_legacy_cases():
    return [(t, K, M, N, mode) for K, M, N, mode, types in MODEL_FORMS_LEGACY for t in types]


# ---- the keys the closure test (tests/test_mm_coverage_cpu.py) named beyond that table, each with the smallest shape found for it (test_model_forms_further)
MODEL_FORMS_FURTHER = [
    (4544, 32741, 17, "default", (Q5_0, Q5_1, Q8_0)),      # two passes at S = 2: the resident form at NBW 2 (Q5_0, Q5_1), k_gemm_skinny<Q8_0, 2>
    (6144, 32741, 17, "default", (Q4_1, Q5_0)),            # .. k_gemm_skinny<T, 2> of the two formats the table leaves out
    (4544, 8229, 17, "default", (Q4_1, Q5_0, Q5_1)),       # two passes of the looping resident form at NBW 2 (Q4_1: NBW 2 at S = 4)
    (4544, 8229, 17, "seq", (Q5_1, Q8_0)),                 # .. at S = 1
    (8192, 1040, 17, "default", LEGACY),                   # two passes of the K-share form at 1 < T < 8, NBW 3
    (18176, 4544, 17, "default", (Q5_0, Q5_1, Q8_0)),      # .. NBW 2
    (8192, 8192, 17, "default", LEGACY),                   # .. at T = 8
    (12288, 8208, 5, "default", (Q4_1,)),                  # Q4_1, 384 blocks (Falcon-180B's Wqkv has 464): T = 8, NBW 2, 65 row blocks on 64 slots
    (12288, 8208, 17, "default", (Q4_1,)),
    (2048, 32752, 5, "default", (Q4_K, Q5_K)),             # the k-quants' streaming forms at S = 2 (lm_head, Falcon-40B's Wup): one K segment ..
    (2048, 32752, 17, "default", (Q4_K, Q5_K)),
    (8448, 32752, 5, "default", (Q4_K, Q5_K)),             # .. two (33 super-blocks)
    (8448, 32752, 17, "default", (Q4_K, Q5_K)),
    (4352, 32752, 5, "default", (Q2_K, Q3_K, Q6_K)),       # .. two of 16 super-blocks (17)
    (4352, 32752, 17, "default", (Q2_K, Q3_K, Q6_K)),
    (2304, 32752, 5, "default", (Q4_K,)),                  # k_gemm_skinny_q4k<Q4_K, 2> at S = 2 with more row blocks than slots (Falcon-40B's Wup)
    (2304, 32752, 17, "default", (Q4_K,)),
    (16640, 3856, 17, "default", (Q4_K,)),                 # several segments, the walk, two passes (Falcon-7B's Wdown, 71 super-blocks)
    (16640, 656, 17, "default", (Q5_K,)),
    (4352, 10752, 17, "default", (Q2_K,)),                 # k_gemm_skinny_q2k<Q2_K, 2>, two segments, every row block on a slot, two passes
    (12544, 16384, 5, "default", (Q2_K,)),                 # .. four segments on 64 slots each: the walk (Falcon-40B's Wdown has eight)
    (12544, 16384, 17, "default", (Q2_K,)),
    (8448, 16384, 17, "default", (Q3_K, Q6_K)),            # .. of Q3_K and Q6_K
    (4352, 16384, 33, "default", (Q2_K, Q3_K)),            # three passes at S = 2 (1024 tiles at 33 columns), NBW 2
    (4352, 8192, 97, "default", (Q2_K,)),                  # seven passes at S = 2 (1024 tiles at 97 columns), NBW 3
]


def model_forms_further_cases():
    return [(t, K, M, N, mode) for K, M, N, mode, types in MODEL_FORMS_FURTHER for t in types]


# ---- the tile GEMM on matrices of whole 64-row workgroups, as every model matrix is (the shapes above have ragged last tiles on purpose): one, whole and ragged
# token tiles per cfg (test_tile_forms_even). mode -> the N it runs at K = 512, M = 128, every format
TILE_FORMS_EVEN_KM = (512, 128)
TILE_FORMS_EVEN = {
    "default": [33, 64, 80, 128, 129],      # k_gemm_q<4, 2> (33, 64) and <4, 4>
    "seq": [33, 128, 129],                  # SEQ16 of the legacy formats up to 128 columns, <1, 4> beyond and for the k-quants
    "cfg3": [33, 128, 129],                 # <2, 4>: what 4 x #CU tiles and more take
    "cfg6": [112, 128, 129],                # <2, 4, 2>: 64-row workgroups
}


def tile_forms_even_cases():
    return [(t, *TILE_FORMS_EVEN_KM, N, mode) for mode, ns in TILE_FORMS_EVEN.items() for N in ns for t in WEIGHT_TYPES]


def op_level_cases():
    """every (type, K, M, N, mode) the op-level GPU tests run, as they parametrize it from the lists above"""
    out = []
    for t in WEIGHT_TYPES:
        legacy = t in LEGACY
        ok = lambda K: K % BLCK[t] == 0        # noqa: E731 (the k-quants skip rows that hold no whole super-blocks)
        out += [(t, K, M, N, "default") for K, M in MUL_MAT_KM for N in MUL_MAT_N if ok(K)]
        for K, M, N in PREFILL_GEMM:
            if ok(K):
                out += [(t, K, M, N, mode) for mode in ("default", "seq", "ref1")]
        for cfg in (6, 7) if legacy else (6,):
            out += [(t, K, M, N, f"cfg{cfg}") for K, M, N in ROWS64 if ok(K)]
        out += [(t, MAT_VEC[0], MAT_VEC[1], N, "default") for N in MAT_VEC[2]]
        out += [(t, K, M, N, "default") for K, M, N in (LEGACY_FORMS if legacy else KQUANT_FORMS)]
        out += [(t, *TILE_INSTANTIATION, f"cfg{c}") for c in (LEGACY_TILE_CFGS if legacy else KQUANT_TILE_CFGS)]
        if legacy:
            out += [(t, *SINGLE_SUM_TILE, "cfg0"), (t, *SEQ16, "seq")]
        out += [(t, K, M, N, mode) for mode in ORDER_MODES for K, M, N in ORDER_SHAPES["legacy" if legacy else "kquant"]]
        out += [(t, K, M, N, mode) for K in (FEW_K_LEGACY if legacy else FEW_K_KQUANTS) for M in FEW_M for N in FEW_N for mode in ("default", "seq")]
    for t in Q4K_SMALL_BATCH_TYPES:
        out += [(t, K, M, N, mode) for K, M, N in Q4K_SMALL_BATCH for mode in ("default", "seq")]
    return out + model_forms_legacy_cases() + model_forms_further_cases() + tile_forms_even_cases()
