"""CPU: code size of the decode launches' plain instantiations (Falcon-7B Q4_0), read from the gfx950 code objects inside the built library.

This is a pin against the text growing back -- debug aids, unused consumer loops and give-up paths creeping into the instantiation that a decode step
launches 32 times per token -- and NOT a performance claim: what the sizes are worth is measured on the GPU (NOTEBOOK, "instruction supply").
The budgets (tests/hot_kernel_budgets.json) are the sizes reached when the instantiations were split, rounded up to the next 2 KiB; each is below the
size the same kernel had before the split (listed beside it). Symbol sizes only: no instruction is decoded."""
import json
import os
import struct

import ggllm_cpp_amd as g

HERE = os.path.dirname(os.path.abspath(__file__))
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _elf_func_sizes(elf):
    """{name: st_size} of the FUNC symbols of a little-endian ELF64 image"""
    assert elf[:4] == b"\x7fELF" and elf[4] == 2 and elf[5] == 1
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    out = {}
    for s in secs:
        if s[1] != 2:                                   # SHT_SYMTAB
            continue
        stroff = secs[s[6]][4]
        for o in range(s[4], s[4] + s[5], 24):
            name, info, _other, _shndx, _value, size = struct.unpack_from("<IBBHQQ", elf, o)
            if info & 0xF == 2:                         # STT_FUNC
                end = elf.index(b"\0", stroff + name)
                out[elf[stroff + name:end].decode()] = size
    return out


def _gfx950_func_sizes(path):
    blob = open(path, "rb").read()
    sizes = {}
    at = blob.find(MAGIC)
    while at >= 0:
        n, = struct.unpack_from("<Q", blob, at + len(MAGIC))
        off = at + len(MAGIC) + 8
        for _ in range(n):
            o, sz, tl = struct.unpack_from("<QQQ", blob, off)
            triple = blob[off + 24:off + 24 + tl]
            off += 24 + tl
            if sz and triple.endswith(b"gfx950"):
                sizes.update(_elf_func_sizes(blob[at + o:at + o + sz]))
        at = blob.find(MAGIC, at + 1)
    return sizes


def test_plain_decode_instantiations_stay_within_their_code_budgets():
    g.build()
    budgets = json.load(open(os.path.join(HERE, "hot_kernel_budgets.json")))
    sizes = _gfx950_func_sizes(g.LIB_PATH)
    assert len(budgets) == 5
    for name, b in budgets.items():
        hits = [s for sym, s in sizes.items() if sym.startswith(b["symbol_prefix"])]
        assert len(hits) == 1, f"{name}: {len(hits)} symbols start with {b['symbol_prefix']}"
        assert b["budget_bytes"] % 2048 == 0 and b["budget_bytes"] < b["bytes_before_split"]
        print(f"{name}: {hits[0]} bytes (budget {b['budget_bytes']}, before the split {b['bytes_before_split']})")
        assert hits[0] <= b["budget_bytes"], f"{name}: {hits[0]} bytes of code, budget {b['budget_bytes']}"
