#!/usr/bin/env python3
"""Opcode histogram of the basic blocks of a gfx950 assembly listing that hold at least --min of one opcode (default: the 512
v_qsad_pk_u16_u8 of a full-pel search pass), and each kernel's whole-function totals.  Static counts, no GPU needed.
usage: tools/kernel_resources.sh svt-av1-1_amd/csrc/me_fullpel.hip && python tools/isa_block_histogram.py /tmp/last_kernel.s"""
import argparse
import collections
import re

ap = argparse.ArgumentParser()
ap.add_argument("asm")
ap.add_argument("--opcode", default="v_qsad_pk_u16_u8")
ap.add_argument("--min", type=int, default=512)
ap.add_argument("--totals", action="store_true", help="also print every kernel's whole-function histogram of vector opcodes")
a = ap.parse_args()

func, label, blocks, order = None, None, collections.defaultdict(collections.Counter), []
totals = collections.defaultdict(collections.Counter)
for line in open(a.asm):
    m = re.match(r"^(_Z\w+):", line)
    if m:
        func, label = m.group(1), m.group(1) + " entry"
        continue
    if line.startswith(".Lfunc_end"):
        func = None
        continue
    if func is None:
        continue
    m = re.match(r"^(\.LBB\w+):(.*)", line)
    if m:
        label = f"{func} {m.group(1)}:{m.group(2).rstrip()}"
        continue
    m = re.match(r"^\s+([a-z][a-z0-9_]+)\b", line)
    if m and not line.lstrip().startswith("."):
        if label not in blocks:
            order.append(label)
        blocks[label][m.group(1)] += 1
        totals[func][m.group(1)] += 1

for label in order:
    c = blocks[label]
    if c[a.opcode] < a.min:
        continue
    vec = sum(n for op, n in c.items() if op.startswith("v_"))
    print(f"== {label} instructions {sum(c.values())}, vector {vec}, vector other than {a.opcode} {vec - c[a.opcode]}")
    for op, n in sorted(c.items(), key=lambda t: (-t[1], t[0])):
        print(f"  {op:<27} {n}")
if a.totals:
    for f, c in totals.items():
        vec = sum(n for op, n in c.items() if op.startswith("v_"))
        print(f"== {f} whole function: instructions {sum(c.values())}, vector {vec}")
