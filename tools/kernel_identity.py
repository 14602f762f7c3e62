#!/usr/bin/env python3
"""Are the conv3x3 kernels of two builds the same device code?

  tools/kernel_identity.py OBJDIR_A OBJDIR_B      (basicsr4rs_amd/lib/obj of two builds)

Unbundles the gfx950 code object of every conv3x3*.o on each side and compares the two sides kernel by kernel, keyed
by mangled name, whichever object a kernel is in: its register / LDS / scratch / kernarg metadata and its whole
instruction stream (addresses and the padding after a kernel dropped).  Prints one summary; exit status 1 on any
difference.  The check for a refactor that only moves kernels between sources.
"""
import glob, os, re, subprocess, sys, tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
        ".kernarg_segment_size", ".max_flat_workgroup_size")
PAD = re.compile(r"^(\.\.\.|s_nop 0|s_code_end)$")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def kernels_of(obj, tmp):
    """{mangled name: (metadata dict, [instruction lines])} of one host object with an embedded fat binary"""
    fb, co = os.path.join(tmp, "fb"), os.path.join(tmp, "co")
    if ".hip_fatbin" not in run(f"{LLVM}/llvm-readelf", "-S", obj):
        return {}  # a host-only source
    run(f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fb}", obj, os.path.join(tmp, "unused.o"))
    run(f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={fb}", f"--output={co}")
    meta, cur = {}, None
    for line in run(f"{LLVM}/llvm-readelf", "--notes", co).splitlines():
        m = re.match(r"^  (- |  )(\.\w+):\s*(.*)$", line)  # the keys of a kernel's own map, not of its .args
        if not m:
            continue
        if m.group(1) == "- ":
            cur = {}
        if m.group(2) == ".name":
            meta[m.group(3)] = cur
        cur[m.group(2)] = m.group(3)
    streams, cur = {}, None
    for line in run(f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = streams.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            cur.append(line.split("//")[0].strip())
    out = {}
    for name, md in meta.items():
        ins = streams[name]
        while ins and PAD.match(ins[-1]):
            ins.pop()
        out[name] = ({k: md.get(k) for k in META}, ins)
    return out


def side(objdir):
    objs = sorted(glob.glob(os.path.join(objdir, "conv3x3*.o")))
    if not objs:
        sys.exit(f"no conv3x3*.o in {objdir}")
    all_k = {}
    with tempfile.TemporaryDirectory() as tmp:
        for o in objs:
            ks = kernels_of(o, tmp)
            dup = set(ks) & set(all_k)
            if dup:
                sys.exit(f"{o}: kernels also in another object: {sorted(dup)[:3]}")
            all_k.update(ks)
            print(f"  {os.path.basename(o):28s} {len(ks):4d} kernels")
    return all_k


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    print(f"A: {sys.argv[1]}")
    a = side(sys.argv[1])
    print(f"B: {sys.argv[2]}")
    b = side(sys.argv[2])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    both = sorted(set(a) & set(b))
    dmeta = [k for k in both if a[k][0] != b[k][0]]
    dins = [k for k in both if a[k][1] != b[k][1]]
    print(f"kernels: A {len(a)}, B {len(b)}; only in A {len(only_a)}, only in B {len(only_b)}")
    print(f"metadata differences: {len(dmeta)}")
    print(f"instruction-stream differences: {len(dins)}")
    print(f"instruction lines: A {sum(len(v[1]) for v in a.values())}, B {sum(len(v[1]) for v in b.values())}")
    for title, names in (("only in A", only_a), ("only in B", only_b), ("metadata differ", dmeta), ("instructions differ", dins)):
        for k in names:
            print(f"  {title}: {k}")
    sys.exit(1 if only_a or only_b or dmeta or dins else 0)


if __name__ == "__main__":
    main()
