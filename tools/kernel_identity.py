#!/usr/bin/env python3
"""Are the kernels of one source family the same device code in two builds?

  tools/kernel_identity.py [--prefix NAME] OBJDIR_A OBJDIR_B      (basicsr4rs_amd/lib/obj of two builds)

Unbundles the gfx950 code object of every NAME*.o (default conv3x3) on each side and compares the two sides kernel
by kernel, whichever object a kernel is in: its register / LDS / scratch / kernarg metadata and its whole
instruction stream (addresses and the padding after a kernel dropped).  A kernel is keyed by its demangled name
without the qualifiers that say only where a name is declared (the anonymous namespace, a family namespace), so that
moving a kernel or an argument struct between namespaces keeps the key.  Prints one summary; exit status 1 on any
difference.  The check for a refactor that only moves kernels between sources.
"""
import argparse, glob, os, re, subprocess, sys, tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
        ".kernarg_segment_size", ".max_flat_workgroup_size")
PAD = re.compile(r"^(\.\.\.|s_nop 0|s_code_end)$")
QUAL = re.compile(r"\(anonymous namespace\)::|\bsr_dcn::")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def kernels_of(obj, tmp):
    """{key: (metadata dict, [instruction lines])} of one host object with an embedded fat binary"""
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
    names = list(meta)
    plain = run("c++filt", *names).splitlines() if names else []
    out = {}
    for name, dem in zip(names, plain):
        ins = streams[name]
        while ins and PAD.match(ins[-1]):
            ins.pop()
        key = QUAL.sub("", dem)
        if key in out:
            sys.exit(f"{obj}: two kernels with the key {key}")
        out[key] = ({k: meta[name].get(k) for k in META}, ins)
    return out


def side(objdir, prefix):
    objs = sorted(glob.glob(os.path.join(objdir, f"{prefix}*.o")))
    if not objs:
        sys.exit(f"no {prefix}*.o in {objdir}")
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
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--prefix", default="conv3x3", help="compare the kernels of PREFIX*.o (default conv3x3)")
    ap.add_argument("objdir_a")
    ap.add_argument("objdir_b")
    args = ap.parse_args()
    print(f"A: {args.objdir_a}")
    a = side(args.objdir_a, args.prefix)
    print(f"B: {args.objdir_b}")
    b = side(args.objdir_b, args.prefix)
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
