"""Compare the gfx950 device code of two builds, kernel by kernel: python scripts/compare_device_code.py OBJDIR_A OBJDIR_B [names]

For every object (default: valuenet distnet tree) the code object is taken out of OBJDIR/<name>.o, disassembled and its
metadata notes read; per kernel the instruction text and the register / scratch / LDS figures of the two builds are compared.
A refactor of host code or of shared device helpers is meant to leave all of them equal.  Exit status 1 on any difference."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin/"
META = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "vgpr_spill_count",
        "sgpr_spill_count", "max_flat_workgroup_size", "kernarg_segment_size")


def code_object(obj, tmp):
    local = os.path.join(tmp, os.path.basename(obj))
    shutil.copy(obj, local)
    subprocess.check_call([LLVM + "llvm-objdump", "--offloading", local], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    cos = [f for f in os.listdir(tmp) if f.startswith(os.path.basename(obj) + ".") and "amdgcn" in f]
    assert cos, "no device code object in " + obj
    return os.path.join(tmp, cos[0])


def kernels(obj):
    """{kernel: (instruction lines, metadata dict)} of the object's gfx950 code object"""
    with tempfile.TemporaryDirectory() as tmp:
        co = code_object(obj, tmp)
        dis = subprocess.check_output([LLVM + "llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co]).decode()
        notes = subprocess.check_output([LLVM + "llvm-readelf", "--notes", co]).decode()
    meta = {}
    for block in notes.split("- .agpr_count:")[1:] if "- .agpr_count:" in notes else notes.split("  - .")[1:]:
        block = ".agpr_count:" + block
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            meta[name.group(1)] = {k: (re.search(r"\.%s:\s+(\d+)" % k, block) or [None, None])[1] for k in META}
    text = {}
    cur = None
    for line in dis.splitlines():
        m = re.match(r"^<(\S+)>:$", line.strip()) or re.match(r"^\S* ?<(\S+)>:$", line)
        if m:
            cur = m.group(1)
            text[cur] = []
        elif cur is not None and line.strip():
            text[cur].append(re.sub(r"\s*//.*$", "", line.strip()))
    assert meta and all(text.get(k) for k in meta), "no kernels read from " + obj      # (an empty comparison must not pass)
    return {k: (text[k], meta[k]) for k in meta}


def main():
    a, b = sys.argv[1], sys.argv[2]
    names = sys.argv[3:] or ["valuenet", "distnet", "tree"]
    bad = 0
    for n in names:
        ka, kb = kernels(os.path.join(a, n + ".o")), kernels(os.path.join(b, n + ".o"))
        if set(ka) != set(kb):
            print("%s: kernel sets differ: %s" % (n, sorted(set(ka) ^ set(kb))))
            bad += 1
        for k in sorted(set(ka) & set(kb)):
            assert ka[k][0], k
            same_text, same_meta = ka[k][0] == kb[k][0], ka[k][1] == kb[k][1]
            print("%-9s %-4s %5d instructions  vgpr %s agpr %s sgpr %s scratch %s lds %s  %s" % (
                n, "same" if same_text and same_meta else "DIFF", len(ka[k][0]), ka[k][1]["vgpr_count"], ka[k][1]["agpr_count"],
                ka[k][1]["sgpr_count"], ka[k][1]["private_segment_fixed_size"], ka[k][1]["group_segment_fixed_size"], k))
            bad += not (same_text and same_meta)
    print("%d difference(s)" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
