"""Compare two builds of one csrc/*.hip kernel by kernel, without a GPU:  python tools/isa_streams.py PARENT.s BRANCH.s

The inputs are the gfx950 assembly files that `hipcc <the Makefile's flags> --save-temps -c FILE.hip` leaves behind
(FILE-hip-amdgcn-amd-amdhsa-gfx950.s).  Per kernel instance: the instruction lines (directives, comments and blank lines
dropped, .LBBn_m labels renumbered in order of appearance) compared as a whole, the instruction count, and SGPRs
(TotalNumSgprs) / VGPRs / scratch bytes from the compiler's own summary.  Verdicts: identical; operands (the same opcodes
in the same order: registers or operand order differ); reordered (the same opcodes in another order); differs.  Kernels
are matched by demangled name; `--map NEW=OLD` pairs a renamed kernel with its predecessor.  Exit status 1 unless every
kernel is identical and has a partner.  Used to hold a refactor to the parent's code (profiles/winograd_transform_refactor.txt)."""
import re
import subprocess
import sys


def demangle(names):
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt"):
        try:
            out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout
            return dict(zip(names, out.split("\n")))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def kernels(path):
    """{mangled name: (instruction lines, sgpr, vgpr, scratch)} of every .amdhsa_kernel in the file"""
    lines = open(path).read().split("\n")
    is_kernel = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", "\n".join(lines), re.M))
    out, name, body, labels = {}, None, [], {}
    for ln in lines:
        s = ln.split(";")[0].rstrip()
        m = re.match(r"^([A-Za-z_][\w.$]*):", s)
        if m and m.group(1) in is_kernel:
            name, body, labels = m.group(1), [], {}
            continue
        if name is None:
            continue
        if s.startswith(".Lfunc_end"):
            out[name] = [body, None, None, None]
            done, name = name, None
            continue
        t = s.strip()
        if not t or (t.startswith(".") and not t.startswith(".LBB")):
            continue
        t = re.sub(r"\.LBB\d+_\d+", lambda k: labels.setdefault(k.group(0), ".L%d" % len(labels)), t)
        body.append(re.sub(r"\s+", " ", t))
    # the compiler's summary comments follow each kernel's descriptor, in the order of the kernels
    order = [n for n in re.findall(r"^([A-Za-z_][\w.$]*):", "\n".join(lines), re.M) if n in out]
    stats = re.findall(r"; TotalNumSgprs: (\d+)\n; NumVgprs: (\d+)(?:\n; [^\n]*)*?\n; ScratchSize: (\d+)", "\n".join(lines))
    assert len(stats) == len(order), "a register summary per kernel expected: %d for %d kernels" % (len(stats), len(order))
    for n, st in zip(order, stats):
        out[n][1:] = [int(v) for v in st]
    return out


def matrix_span_table(path, pattern):
    """`python tools/isa_streams.py --waits REGEX FILE.s`: one row per kernel whose demangled name matches REGEX -- VGPRs,
    spilled VGPRs and scratch bytes (.vgpr_count / .vgpr_spill_count of the metadata, ScratchSize), code bytes
    (codeLenInByte), and between the kernel's first and last MFMA the number of buffer loads and the histogram of the N
    in `s_waitcnt vmcnt(N)`: how many global loads each wait leaves in flight.  A static count over every row-tile
    variant the kernel holds (profiles/rb16s_unrolled_isa.txt)."""
    text = open(path).read()
    K = kernels(path)
    names = demangle(list(K))
    size = dict(re.findall(r"^([A-Za-z_][\w.$]*):.*?\n; codeLenInByte = (\d+)", text, re.M | re.S))
    meta = {n: (int(v), int(sp)) for n, v, sp in
            re.findall(r"\.name:\s+(\S+)\n(?:(?!\.name:).)*?\.vgpr_count:\s+(\d+)\n\s*\.vgpr_spill_count:\s+(\d+)", text, re.S)}
    print("%-46s | VGPR | spill | scratch | code B | loads | vmcnt(N): count, between the first and the last MFMA" % "kernel")
    for k in sorted(K, key=lambda k: names[k]):
        short = re.sub(r"^(void )?nfs::", "", re.sub(r"\(.*$", "", names[k]))
        if not re.search(pattern, short):
            continue
        body = K[k][0]
        mf = [i for i, ln in enumerate(body) if ln.startswith("v_mfma")]
        span = body[mf[0]:mf[-1] + 1] if mf else []
        hist = {}
        for ln in span:
            m = re.match(r"s_waitcnt .*?vmcnt\((\d+)\)", ln)
            if m:
                hist[int(m.group(1))] = hist.get(int(m.group(1)), 0) + 1
        loads = sum(ln.startswith("buffer_load") for ln in span)
        print("%-46s | %4d | %5d | %7d | %6d | %5d | %s" % (
            short, meta[k][0], meta[k][1], K[k][3], int(size[k]), loads,
            " ".join("%d:%d" % (n, c) for n, c in sorted(hist.items()))))
    return 0


def main(argv):
    if len(argv) == 3 and argv[0] == "--waits":
        return matrix_span_table(argv[2], argv[1])
    maps =dict(a.split("=", 1) for i, a in enumerate(argv) if i and argv[i - 1] == "--map")
    files = [a for i, a in enumerate(argv) if a != "--map" and not (i and argv[i - 1] == "--map")]
    if len(files) != 2:
        sys.exit(__doc__)
    P, B = kernels(files[0]), kernels(files[1])
    dp, db = demangle(list(P)), demangle(list(B))
    short = lambda d: re.sub(r"^(void )?nfs::", "", re.sub(r"\(.*$", "", d))
    pn = {short(dp[k]): k for k in P}
    bad = 0
    print("%-52s | %-9s | %-13s | %-22s | %s" % ("kernel", "verdict", "instr", "parent SGPR/VGPR/scr", "new SGPR/VGPR/scr"))
    for k in B:
        n = short(db[k])
        o = pn.pop(maps.get(n, n), None)
        if o is None:
            print("%-52s | NEW" % n)
            bad += 1
            continue
        same = P[o][0] == B[k][0]
        bad += not same
        ops = [[i.split(" ")[0] for i in K[0]] for K in (P[o], B[k])]
        verdict = "identical" if same else "operands" if ops[0] == ops[1] else "reordered" if sorted(ops[0]) == sorted(ops[1]) else "differs"
        print("%-52s | %-9s | %5d -> %5d | %8d / %3d / %3d    | %4d / %3d / %3d" % (
            n if n not in maps else "%s (was %s)" % (n, maps[n]), verdict, len(P[o][0]), len(B[k][0]), *P[o][1:], *B[k][1:]))
    for n in pn:
        print("%-52s | GONE" % n)
        bad += 1
    print("%d kernel instances, %d not identical" % (len(B), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
