"""Code bytes and resource figures of every k_sim_step* kernel in the built library's gfx950 code object:

    python scripts/sim_step_code_size.py [LIB] [--json OUT.json]

LIB defaults to tetris_mcts_amd/libtetris_mcts_hip.so.  The sizes are the symbols' `st_size` (llvm-readelf -sW), the registers,
spills, scratch and LDS the code object's metadata notes.  With --json the table is merged into OUT.json under "code_size"
(the file's other keys are kept)."""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin/")
META = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
        "group_segment_fixed_size")


def sim_step_kernels(lib):
    """{demangled kernel name: {"symbol", "code_bytes", metadata...}} of the k_sim_step* kernels in lib"""
    with tempfile.TemporaryDirectory() as tmp:
        local = os.path.join(tmp, "lib.so")
        shutil.copy(lib, local)
        subprocess.check_call([LLVM + "llvm-objdump", "--offloading", local], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        out = {}
        for co in sorted(f for f in os.listdir(tmp) if f.startswith("lib.so.") and "amdgcn" in f):
            co = os.path.join(tmp, co)
            syms = subprocess.check_output([LLVM + "llvm-readelf", "-sW", co]).decode()
            notes = subprocess.check_output([LLVM + "llvm-readelf", "--notes", co]).decode()
            meta = {}
            for block in notes.split("- .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+(\S+)", block)
                if name:
                    block = ".agpr_count:" + block
                    meta[name.group(1)] = {k: int((re.search(r"\.%s:\s+(\d+)" % k, block) or [0, 0])[1]) for k in META}
            # (the demangled table gives the readable name of the symbol at the same address)
            nice = {}
            for line in subprocess.check_output([LLVM + "llvm-readelf", "-sW", "--demangle", co]).decode().splitlines():
                f = line.split(None, 7)
                if len(f) == 8 and f[3] == "FUNC":
                    nice[f[1]] = re.sub(r"\(.*$", "", f[7]).replace("void ", "").strip()
            for line in syms.splitlines():
                f = line.split()
                if len(f) == 8 and f[3] == "FUNC" and "k_sim_step" in f[7]:
                    out[nice.get(f[1], f[7])] = dict(symbol=f[7], code_bytes=int(f[2]), **meta.get(f[7], {}))
    assert out, "no k_sim_step* kernel in " + lib
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_json = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    if out_json:
        args.remove(out_json)
    lib = args[0] if args else os.path.join(ROOT, "tetris_mcts_amd", "libtetris_mcts_hip.so")
    ks = sim_step_kernels(lib)
    for name, k in sorted(ks.items()):
        print("%-34s %7d bytes  vgpr %s sgpr %s sgpr spills %s vgpr spills %s scratch %s lds %s" % (
            name, k["code_bytes"], k.get("vgpr_count"), k.get("sgpr_count"), k.get("sgpr_spill_count"), k.get("vgpr_spill_count"),
            k.get("private_segment_fixed_size"), k.get("group_segment_fixed_size")))
    if out_json:
        doc = {}
        if os.path.exists(out_json):
            with open(out_json) as f:
                doc = json.load(f)
        doc["code_size"] = ks
        with open(out_json, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    sys.exit(main())
