"""Static comparison of two tracer code objects, kernel by kernel: registers, spills, scratch and
LDS from the code objects' notes, and for kernels whose instruction streams differ the counts of
VALU, scalar ALU (tools/valu_regions.py is_salu), scalar memory and LDS instructions.

  python tools/static_compare.py ab_objs/parent.hsaco ab_objs/new.hsaco
"""
import collections
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import valu_attrib as V  # noqa: E402
from valu_regions import is_salu  # noqa: E402

KEYS = (("vgpr", ".vgpr_count"), ("sgpr", ".sgpr_count"), ("vspill", ".vgpr_spill_count"),
        ("sspill", ".sgpr_spill_count"), ("scratch", ".private_segment_fixed_size"),
        ("lds", ".group_segment_fixed_size"))


def notes(hsaco):
    """kernel name -> {note key: value} from the code object's metadata."""
    out = subprocess.run([f"{V.LLVM}/llvm-readelf", "--notes", hsaco], capture_output=True,
                         text=True, check=True).stdout
    kernels, cur = collections.OrderedDict(), {}
    for line in out.splitlines():
        m = re.match(r"\s*(?:- )?(\.\w+):\s*(\S+)\s*$", line)
        if not m:
            continue
        if line.lstrip().startswith("- ") and ".name" in cur:  # the next list item
            kernels[cur[".name"]] = cur
            cur = {}
        cur[m.group(1)] = m.group(2)
    if ".name" in cur:
        kernels[cur[".name"]] = cur
    return {k: v for k, v in kernels.items() if ".vgpr_count" in v}


def all_disasm(hsaco):
    """kernel -> [instruction text, addresses and literals' values left out]."""
    out = subprocess.run([f"{V.LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", hsaco],
                         capture_output=True, text=True, check=True).stdout
    per, cur = collections.defaultdict(list), None
    for line in out.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\w+)>:", line)
        if m:
            cur = m.group(1)
            continue
        m = re.match(r"^\s+(\S+)(.*?)//\s*[0-9A-F]+:", line)
        if m and cur:
            per[cur].append((m.group(1), re.sub(r"0x[0-9a-f]+", "X", (m.group(1) + m.group(2)).strip())))
    return per


def counts(insts):
    c = collections.Counter()
    for mn, _ in insts:
        c["VALU"] += V.is_valu(mn)
        c["SALU"] += is_salu(mn)
        c["SMEM"] += mn.startswith(("s_load", "s_buffer_load"))
        c["DS"] += mn.startswith("ds_")
    c["len"] = len(insts)
    return c


def main():
    a, b = sys.argv[1:3]
    na, nb = notes(a), notes(b)
    da, db = all_disasm(a), all_disasm(b)
    for k in na:
        if k not in nb:
            print(f"{k}: only in {a}")
            continue
        same = [t for _, t in da[k]] == [t for _, t in db[k]]
        line = f"{k}: {'SAME' if same else 'DIFF'} " + " ".join(
            f"{n} {na[k].get(key, '?')}->{nb[k].get(key, '?')}" for n, key in KEYS)
        if not same:
            ca, cb = counts(da[k]), counts(db[k])
            line += " " + " ".join(f"{n} {ca[n]}->{cb[n]}" for n in ("len", "VALU", "SALU", "SMEM", "DS"))
        print(line)
    for k in nb:
        if k not in na:
            print(f"{k}: only in {b}")


if __name__ == "__main__":
    main()
