#!/usr/bin/env python3
"""Compares the gfx950 device code of two builds, kernel by kernel.

    python tools/device_code_diff.py OLD_OBJ_DIR NEW_OBJ_DIR [object names ...]

Both directories hold the objects ``fastspeech2_lightning_amd.build`` leaves in ``fastspeech2_lightning_amd/build/``.
Without names every object present in both directories is compared (one that only one of them has is named, nothing
more); the name ``gemm-family`` stands for the eight GEMM objects.  From every object the gfx950 code object is taken
out of the ``.hip_fatbin`` section (llvm-objcopy, clang-offload-bundler) and disassembled (llvm-objdump -d); the two
disassemblies are compared PER SYMBOL -- the order in which templates are first used may reorder the kernels inside a
code object, so addresses are dropped and only each symbol's instruction text and encodings count (zero padding behind a
symbol's last instruction is dropped too).  Prints one line per object; exits non-zero when a symbol is missing on
either side or its instructions differ.  A host-side refactor must come out identical."""
from __future__ import annotations

import os
import re
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

GEMM_OBJECTS = ["gemm", "gemm2", "gemm2p", "gemm_bf16", "gemm_bf16p", "gemm_ws", "gemm_ws4", "gemm_ws32"]
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def tool(name: str) -> str:
    for d in (os.environ.get("LLVM_BIN"), str(Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "llvm" / "bin")):
        if d and (Path(d) / name).exists():
            return str(Path(d) / name)
    found = shutil.which(name)
    if not found:
        raise SystemExit(f"{name} not found (set LLVM_BIN or ROCM_PATH)")
    return found


def disassemble(obj: Path, tmp: Path) -> dict[str, list[str]]:
    """{symbol: [instruction text + encoding, ...]} of the object's gfx950 code object"""
    fatbin, co = tmp / (obj.stem + ".fatbin"), tmp / (obj.stem + ".co")
    sections = subprocess.run([tool("llvm-objdump"), "-h", str(obj)], check=True, capture_output=True, text=True).stdout
    if ".hip_fatbin" not in sections:  # a host-only source
        return {}
    subprocess.run([tool("llvm-objcopy"), f"--dump-section=.hip_fatbin={fatbin}", str(obj)], check=True)
    subprocess.run([tool("clang-offload-bundler"), "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={fatbin}",
                    f"--output={co}"], check=True)
    text = subprocess.run([tool("llvm-objdump"), "-d", str(co)], check=True, capture_output=True, text=True).stdout
    # every symbol's address, for the pc-relative references below
    table = subprocess.run([tool("llvm-objdump"), "-t", str(co)], check=True, capture_output=True, text=True).stdout
    placed = sorted((int(m.group(1), 16), m.group(3)) for m in
                    re.finditer(r"^([0-9a-f]{16}) .{7} (\S+)\t[0-9a-f]{16} (?:\.\w+ )?(\S+)$", table, flags=re.M)
                    if not m.group(2).startswith("*"))

    def where(addr: int) -> str:
        below = [(a, n) for a, n in placed if a <= addr]
        return f"{below[-1][1]}+{addr - below[-1][0]:#x}" if below else f"{addr:#x}"

    symbols: dict[str, list[str]] = {}
    cur = None
    getpc = None  # register pair of an s_getpc_b64 on the previous line
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = symbols.setdefault(m.group(1), [])
            continue
        if cur is None or not line.startswith(("\t", " ")) or not line.strip():
            continue
        if line.strip() == "...":  # zero padding up to the next symbol's alignment: depends on which kernel follows
            continue
        insn, _, note = line.partition("//")
        # the note is "<address>: <encoding words> [<symbol+offset>]": keep the encoding, drop where the code landed
        enc = " ".join(re.sub(r"<[^>]*>", "", note.partition(":")[2]).split())
        insn = " ".join(insn.split())
        # "s_getpc_b64 s[n:n+1]; s_add_u32 sn, sn, literal" is the address of a global (pc + literal, pc = this
        # instruction): the literal depends on where the kernel was placed, the global it reaches does not
        m = re.match(r"s_add_u32 (s\d+), \1, (0x[0-9a-f]+|\d+)$", insn)
        if m and getpc == m.group(1):
            lit = int(m.group(2), 0)
            target = int(note.partition(":")[0], 16) + (lit - (1 << 32) if lit >= 1 << 31 else lit)
            insn, enc = f"s_add_u32 {getpc}, {getpc}, @{where(target)}", enc.split()[0]
        g = re.match(r"s_getpc_b64 s\[(\d+):\d+\]$", insn)
        getpc = f"s{g.group(1)}" if g else None
        cur.append(insn + " | " + enc)
    for insns in symbols.values():  # a single zero word of the same padding is printed as an instruction, not as "..."
        while insns and insns[-1].endswith("| 00000000"):
            insns.pop()
    return symbols


def main(argv: list[str]) -> int:
    if len(argv) < 3:
        print(__doc__)
        return 2
    old, new = Path(argv[1]), Path(argv[2])
    names = [n for arg in argv[3:] for n in (GEMM_OBJECTS if arg == "gemm-family" else [arg])]
    bad = 0
    if not names:
        have = [{p.stem for p in d.glob("*.o")} for d in (old, new)]
        names = sorted(have[0] & have[1])
        for only in sorted(have[0] ^ have[1]):
            print(f"{only}: in one build only, not compared")
    with tempfile.TemporaryDirectory() as t:
        (Path(t) / "old").mkdir()
        (Path(t) / "new").mkdir()
        for name in names:
            a = disassemble(old / f"{name}.o", Path(t) / "old")
            b = disassemble(new / f"{name}.o", Path(t) / "new")
            missing, added = sorted(set(a) - set(b)), sorted(set(b) - set(a))
            differ = sorted(s for s in set(a) & set(b) if a[s] != b[s])
            n_insn = sum(len(v) for v in b.values())
            if missing or added or differ:
                bad += 1
                print(f"{name}: DIFFERENT -- {len(missing)} symbols gone, {len(added)} new, {len(differ)} changed "
                      f"(of {len(a)} / {len(b)})")
                for label, syms in (("gone", missing), ("new", added), ("changed", differ)):
                    for s in syms[:10]:
                        print(f"    {label}: {s}")
            else:
                print(f"{name}: identical -- {len(b)} symbols, {n_insn} instructions" if b else f"{name}: no device code")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
