#!/usr/bin/env python3
"""Kernel identity of gfx950 code objects across a split or move of a HIP unit: the kernels of the old
objects against those of the new ones -- (a) names, (b) the resource notes of llvm-readelf --notes, (c) the
instruction streams of llvm-objdump -d without addresses, encodings and branch targets.
usage: tools/kernel_identity.py OUT.txt OLD.o [OLD2.o ...] -- NEW1.o [NEW2.o ...]      (ROCM: /opt/rocm)"""
import difflib, os, re, subprocess, sys, tempfile
LLVM = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "llvm", "bin")
KEYS = [".vgpr_count", ".sgpr_count", ".agpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
        ".vgpr_spill_count", ".sgpr_spill_count"]

def code_object(obj, tmp):
    base = os.path.join(tmp, os.path.basename(os.path.dirname(os.path.dirname(obj))) + "_" + os.path.basename(obj))
    fb, co = base + ".fatbin", base + ".co"
    subprocess.check_call([LLVM + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + fb, obj])
    subprocess.check_call([LLVM + "/clang-offload-bundler", "--unbundle", "--type=o",
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fb, "--output=" + co])
    return co

def notes(co):
    out = subprocess.check_output([LLVM + "/llvm-readelf", "--notes", co], text=True)
    res = {}
    for blk in re.split(r"\n  - (?=\.)", out[out.index("amdhsa.kernels:"):]):
        top = "\n".join(l for l in ("    " + blk).split("\n") if re.match(r"^    \.[a-z_]+:", l))
        m = re.search(r"\.name:\s+(\S+)", top)
        if not m: continue
        d = {}
        for k in KEYS:
            d[k] = int(re.search(r"    " + re.escape(k) + r":\s+(\d+)", top).group(1))
        res[m.group(1)] = d
    return res

def streams(co, names):
    out = subprocess.check_output([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co], text=True)
    res, cur = {}, None
    for line in out.split("\n"):
        m = re.match(r"^[0-9a-f]* ?<(.+)>:$", line.strip())
        if m:
            cur = m.group(1) if m.group(1) in names else (cur if m.group(1).startswith("L") or m.group(1).startswith(".L") else None)
            if m.group(1) in names: res[cur] = []
            continue
        if cur is None or not line.strip() or line.strip() == "...": continue
        t = line.split("//")[0].strip()
        t = re.sub(r"<[^>]*>", "<sym>", t)
        # pc-relative operands: branch targets and the literals of s_getpc / s_add_u32 address arithmetic
        if re.match(r"s_(c?branch|call)", t): t = re.sub(r"\s\S+$", " <target>", t)
        res[cur].append(t)
    return res

def main():
    out = sys.argv[1]
    i = sys.argv.index("--")
    parent, new = sys.argv[2:i], sys.argv[i + 1:]
    tmp = tempfile.mkdtemp()
    def load(objs):
        N, S, where = {}, {}, {}
        for o in objs:
            co = code_object(o, tmp)
            n = notes(co)
            s = streams(co, set(n))
            for k in n:
                assert k not in N, "kernel %s in two objects" % k
                N[k] = n[k]; S[k] = s.get(k, []); where[k] = os.path.basename(o)
        return N, S, where
    PN, PS, PW = load(parent)
    NN, NS, NW = load(new)
    L = []
    L.append("kernel identity, gfx950 code objects: parent %s against %s" % (", ".join(map(os.path.basename, parent)), ", ".join(map(os.path.basename, new))))
    L.append("parent kernels: %d (band: %d)   new kernels: %d  (%s)" % (
        len(PN), sum(1 for k in PN if re.search(r"k_bj|k_scatter", k)), len(NN),
        ", ".join("%s %d" % (o, sum(1 for k in NW if NW[k] == o)) for o in sorted(set(NW.values())))))
    L.append("(a) names: only in parent %d, only in new %d" % (len(set(PN) - set(NN)), len(set(NN) - set(PN))))
    for k in sorted(set(PN) ^ set(NN)): L.append("    %s" % k)
    bad_b = [k for k in PN if k in NN and PN[k] != NN[k]]
    L.append("(b) resource notes (%s): %d kernels differ" % (" ".join(KEYS), len(bad_b)))
    for k in bad_b: L.append("    %s: %s -> %s" % (k, PN[k], NN[k]))
    bad_c = [k for k in PN if k in NN and PS[k] != NS[k]]
    L.append("(c) instruction streams (llvm-objdump -d, addresses, encodings and branch targets stripped): %d kernels differ" % len(bad_c))
    for k in bad_c:
        d = [x for x in difflib.unified_diff(PS[k], NS[k], lineterm="", n=0) if x[0] in "+-" and not x.startswith(("+++", "---"))]
        L.append("    %s: %d / %d instructions, %d diff lines" % (k, len(PS[k]), len(NS[k]), len(d)))
        for x in d[:20]: L.append("        " + x)
    L.append("")
    L.append("%-8s %-12s %5s %5s %5s %7s %7s %6s %6s %8s  %s" % ("same", "unit", "vgpr", "sgpr", "agpr", "lds", "scratch", "vspill", "sspill", "insts", "kernel"))
    for k in sorted(PN):
        n = NN.get(k)
        ok = n is not None and n == PN[k] and PS[k] == NS[k]
        p = PN[k]
        L.append("%-8s %-12s %5s %5s %5s %7s %7s %6s %6s %8d  %s" % ("yes" if ok else "NO", NW.get(k, "-"), p[KEYS[0]], p[KEYS[1]], p[KEYS[2]], p[KEYS[3]],
                 p[KEYS[4]], p[KEYS[5]], p[KEYS[6]], len(PS[k]), k))
    open(out, "w").write("\n".join(L) + "\n")
    print("\n".join(L[:8 + len(bad_b) + len(bad_c) * 4]))

main()
