"""falcon_main's context swap (examples/falcon/falcon_main.cpp:694-751), restated in Python for tests/test_ctx_swap_cpu.py and
tests/test_gpu_ctx_swap.py, and the cases of tests/golden/ctx_swap.npz (written by tests/gen_ctx_swap_golden.py)."""

CLI_PROMPT = "The quick brown fox didn't jump"                          # 11 tokens of the tiny BPE model (oracle/gen_golden.py)
P25 = CLI_PROMPT + " over the lazy dog and then ran away"              # 25 tokens
SYSTEM = "Be terse. "
COMMON = ["-c", "32", "-t", "2", "--ignore-eos"]                        # every case; -b and -s per case
N_CTX = 32

# name -> (prompt, n_predict, n_batch, seed, keep, system prompt or None, sampler flags as falcon_main takes them)
CASES = {
    "p_keep0":        (CLI_PROMPT, 80, 8, 1, 0, None, ["--temp", "0"]),
    "p_keep6":        (CLI_PROMPT, 80, 8, 1, 6, None, ["--temp", "0"]),
    "p_temp_keepall": (CLI_PROMPT, 80, 8, 1, -1, None, ["--temp", "0.8"]),
    "p25_keep0":      (P25, 40, 8, 1, 0, None, ["--temp", "0"]),
    "p25_keepall":    (P25, 40, 8, 1, -1, None, ["--temp", "0"]),
    "sys_mirostat2":  (CLI_PROMPT, 60, 8, 1, 4, SYSTEM, ["--mirostat", "2"]),
    "p_tfs_typical":  (CLI_PROMPT, 80, 8, 1, 0, None, ["--tfs", "0.9", "--typical", "0.9"]),
    "p_b4":           (CLI_PROMPT, 80, 4, 1, 0, None, ["--temp", "0"]),
}


def main_args(name):
    """falcon_main's arguments of a case, without -m and the model"""
    prompt, n_predict, n_batch, seed, keep, system, flags = CASES[name]
    a = ["-p", prompt, "-n", str(n_predict), "-b", str(n_batch), "-s", str(seed), "--keep", str(keep), *COMMON, *flags]
    if system is not None:
        a += ["-sys", system, "-sysraw"]
    return a


def kept(n_ctx, n_system, n_keep, prompt_size):
    """rows of the cache that survive a swap (falcon_main.cpp:524, 712-718)"""
    if n_keep < 0 or n_keep > prompt_size:
        n_keep = prompt_size
    nk = n_system
    if n_keep > 0 and prompt_size > n_system:
        nk += min(n_keep, prompt_size - n_system)
    return nk


def plan(n_ctx, n_system, n_keep, prompt_size, n_history, n_pending=1):
    """(n_past_new, n_regen) of a swap (falcon_main.cpp:719-729)"""
    nk = kept(n_ctx, n_system, n_keep, prompt_size)
    if nk < n_ctx // 2:
        n_regen = n_ctx // 2 - nk
    elif nk < n_ctx - 10:
        n_regen = 4
    else:
        n_regen = 0
    return nk, min(n_regen, n_history - n_pending)


def prompt_history(prompt, n_batch):
    """what a prompt leaves in all_generation: the last token of every batch (falcon_main.cpp:1013-1021, 1054-1055)"""
    return [prompt[min(i + n_batch, len(prompt)) - 1] for i in range(0, len(prompt), n_batch)]


def replay(prompt, drawn, n_ctx, n_batch, n_keep, n_system=0):
    """falcon_main's loop over a known token stream: the swaps it makes while it draws `drawn` after `prompt` (the system tokens first) --
    [(n_past_new, [regenerated ids..., the pending id])], the id lists being what --verbose-prompt prints between #CONTEXT_RESET_START and #RESET_END"""
    hist = prompt_history(list(prompt), n_batch)
    n_past, blocks = len(prompt), []
    for i, t in enumerate(drawn):
        hist.append(t)
        if i + 1 == len(drawn):
            break                                            # (the last draw is printed, never evaluated)
        if n_past + 1 > n_ctx:
            nk, nr = plan(n_ctx, n_system, n_keep, len(prompt), len(hist))
            blocks.append((nk, hist[len(hist) - 1 - nr:]))
            n_past = nk + nr
        n_past += 1
    return blocks
