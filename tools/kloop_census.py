#!/usr/bin/env python3
"""Instruction census of conv_wino_f32_kernel's K loop from hipcc's assembly (-S, device only).

The K loop is the innermost loop of the <false> kernel with 64 v_mfma (two chunks).
Per chunk and per group of four MFMAs it prints how many instructions of each class stand ahead
of the group's first MFMA and between its MFMAs (`a|b|c|d` = before MFMA 0 | between 0 and 1 |
1 and 2 | 2 and 3), then the totals per chunk and whether packed f32 arithmetic occurs.

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include --cuda-device-only -S csrc/conv_wino_f32.hip -o wino.s
  python tools/kloop_census.py wino.s
"""
import collections
import re
import sys

CLASSES = ("VALU", "ds_read", "ds_write", "VMEM load", "LDS-DMA", "SALU", "s_waitcnt", "other")


def classify(op, rest):
    if op.startswith("v_mfma"):
        return "MFMA"
    if op.startswith("s_waitcnt"):
        return "s_waitcnt"
    if op.startswith("ds_read") or op.startswith("ds_load"):
        return "ds_read"
    if op.startswith("ds_write") or op.startswith("ds_store"):
        return "ds_write"
    if op.startswith(("buffer_load", "global_load")):
        return "LDS-DMA" if re.search(r"\blds\b", rest) or "_lds_" in op else "VMEM load"
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("s_") and not op.startswith(("s_barrier", "s_nop", "s_cbranch", "s_branch", "s_setprio")):
        return "SALU"
    return "other"


def loop_body(path, kernel):
    """Instructions of the innermost loop that holds 64 MFMAs: the span of the shortest backward
    branch with that many (the odd chunk's uniform branch splits the body into several blocks)."""
    ins, labels, inside = [], {}, False
    for line in open(path):
        s = line.split(";")[0].strip()
        if s.startswith(kernel + ":"):
            inside = True
            continue
        if not inside or not s:
            continue
        if s.startswith(".Lfunc_end"):
            break
        m = re.match(r"^(\.?[A-Za-z_0-9$]+):$", s)
        if m:
            labels[m.group(1)] = len(ins)
            continue
        if s.startswith("."):
            continue
        parts = s.split(None, 1)
        ins.append((parts[0], parts[1] if len(parts) > 1 else ""))
    best = None
    for i, (op, rest) in enumerate(ins):
        if op.startswith(("s_cbranch", "s_branch")) and labels.get(rest.strip(), i + 1) <= i:
            span = ins[labels[rest.strip()]:i + 1]
            if sum(o.startswith("v_mfma") for o, _ in span) == 64 and (best is None or len(span) < len(best)):
                best = span
    if best is None:
        sys.exit("no loop with 64 MFMAs found")
    return best


def main():
    path = sys.argv[1]
    kernel = sys.argv[2] if len(sys.argv) > 2 else "_ZN4eosv20conv_wino_f32_kernelILb0EEEvNS_8WinoArgsE"
    body = loop_body(path, kernel)
    nm = sum(o.startswith("v_mfma") for o, _ in body)
    print(f"K loop: {len(body)} instructions, {nm} MFMAs ({nm // 32} chunks)")
    segs, cur = [], collections.Counter()   # one counter per MFMA: what stands ahead of it
    packed, waits = collections.Counter(), []
    for op, rest in body:
        c = classify(op, rest)
        if op.startswith(("v_pk_add_f32", "v_pk_mul_f32", "v_pk_fma_f32")):
            packed[op] += 1
        if c == "s_waitcnt":
            waits.append(rest)
        if c == "MFMA":
            segs.append(cur)
            cur = collections.Counter()
        else:
            cur[c] += 1
    tail = cur
    for ch in range(nm // 32):
        print(f"-- chunk {ch} of the unrolled pair")
        tot = collections.Counter()
        for g in range(8):
            ss = segs[ch * 32 + 4 * g: ch * 32 + 4 * g + 4]
            cells = []
            for c in CLASSES:
                if any(s[c] for s in ss):
                    cells.append(f"{c} " + "|".join(str(s[c]) for s in ss))
            for s in ss:
                tot.update(s)
            print(f"  group {g}: " + ("; ".join(cells) or "nothing"))
        print("  chunk total (MFMAs 32): " + ", ".join(f"{c} {tot[c]}" for c in CLASSES))
    print("after the last MFMA (barrier, loop control): " + ", ".join(f"{c} {tail[c]}" for c in CLASSES if tail[c]))
    print("s_waitcnt operands in order: " + " / ".join(waits))
    print("packed f32 arithmetic: " + (", ".join(f"{k} x{v}" for k, v in packed.items()) or "none"))
    ops = collections.Counter(o for o, _ in body)
    print("opcodes: " + ", ".join(f"{k} {v}" for k, v in sorted(ops.items(), key=lambda kv: -kv[1])))


if __name__ == "__main__":
    main()
