"""Kernel-by-kernel ISA comparison of two builds of audioldm2_amd/csrc (e.g. a parent commit and a branch): every kernel function of
the gfx950 code object in each object's .hip_fatbin is disassembled (llvm-objdump -d --no-show-raw-insn) and compared instruction by
instruction, with comments and branch-target labels stripped.  A renamed instantiation can be matched with --rename OLD=NEW
(substring replacement on the mangled name of the first build).
Usage: python tools/isa_compare.py <csrc dir A> <csrc dir B> [--rename OLD=NEW ...] [--objs attn igemm ...]
Prints, per object, the number of identical and differing functions and the functions only one side has; exit 1 if any differ.
Example (the TAIL template argument of attention_d32_presplit2_kernel, v10):
  python tools/isa_compare.py parent/audioldm2_amd/csrc audioldm2_amd/csrc \\
      --rename ELb0EEEvPKfPKvS4_=ELb0ELb0EEEvPKfPKvS4_ --rename ELb1EEEvPKfPKvS4_=ELb1ELb0EEEvPKfPKvS4_"""
import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")


def disasm(obj):
    """{mangled kernel name: [instructions]} of the gfx950 code object of one .o ({} for an object without device code)."""
    with tempfile.TemporaryDirectory() as d:
        fb, co = os.path.join(d, "fb.bin"), os.path.join(d, "co")
        if subprocess.call([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fb}", obj, os.path.join(d, "x")],
                           stderr=subprocess.DEVNULL) != 0:
            return {}
        targets = subprocess.check_output([f"{LLVM}/clang-offload-bundler", "--list", "--type=o", f"--input={fb}"], text=True)
        t = [x for x in targets.split() if "gfx950" in x][0]
        subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--type=o", f"--targets={t}", f"--input={fb}", f"--output={co}",
                               "--unbundle"])
        text = subprocess.check_output([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co], text=True)
    funcs, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^<(.+)>:$", line.strip())
        if m:
            cur = m.group(1)
            funcs[cur] = []
        elif cur and line.strip():
            funcs[cur].append(re.sub(r"<[^>]*>", "", re.sub(r"//.*", "", line)).strip())
    return funcs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--rename", action="append", default=[])
    ap.add_argument("--objs", nargs="*", default=None)
    args = ap.parse_args()
    ren = [r.split("=", 1) for r in args.rename]
    objs = args.objs or sorted(os.path.basename(p)[:-2] for p in glob.glob(os.path.join(args.a, "*.o")) if not p.endswith(".th.o"))
    bad = False
    for o in objs:
        fa, fb = disasm(os.path.join(args.a, o + ".o")), disasm(os.path.join(args.b, o + ".o"))
        same, diff, matched = 0, [], set()
        for k, ins in fa.items():
            kb = k
            if kb not in fb:
                for old, new in ren:
                    kb = kb.replace(old, new)
            if kb not in fb:
                continue
            matched.add(kb)
            if ins == fb[kb]:
                same += 1
            else:
                diff.append(k)
        only_a = [k for k in fa if k not in fb and all(k.replace(o_, n_) not in fb for o_, n_ in ren)]
        only_b = [k for k in fb if k not in matched]
        print(f"{o}: identical {same}  differing {len(diff)}  only in A {len(only_a)}  only in B {len(only_b)}")
        for k in diff:
            print("   differs:", k)
        for k in only_b:
            print("   new:", k)
        bad = bad or bool(diff)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
