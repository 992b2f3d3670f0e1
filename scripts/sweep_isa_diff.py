"""Are the two tuned BBPGD sweeps the same machine code in two builds of convex.hip?

    python scripts/sweep_isa_diff.py PARENT.s HEAD.s

PARENT.s / HEAD.s: the gfx950 device assembly of convex.hip of two trees, compiled with the flags of
mundy_amd/build.py plus --save-temps (convex-hip-amdgcn-amd-amdhsa-gfx950.s).  For every instantiation of
mhip::k_body<...> and mhip::k_constraint<...> the instruction text (comments dropped, the function's local label
numbers normalised) and the .amdhsa_* kernel descriptor (registers, LDS, scratch) are compared.  One line per kernel;
exit status 1 if any differs or exists in one file only.  CPU only."""
import re
import sys

HOT = ("_ZN4mhip6k_bodyI", "_ZN4mhip12k_constraintI")  # mhip::k_body<, mhip::k_constraint<


def kernels(path):
    """symbol -> (instruction lines, descriptor lines) of the hot kernels of one assembly file"""
    out, sym, part = {}, None, None
    for ln in open(path):
        m = re.search(r"; -- Begin function (\S+)", ln)
        if m:
            sym = m.group(1) if m.group(1).startswith(HOT) else None
            part = None
            if sym:
                out[sym] = ([], [])
            continue
        if sym is None:
            continue
        if "; -- End function" in ln:
            sym = None
            continue
        s = ln.split(";")[0].strip()
        if s == sym + ":":
            part = 0
        elif s.startswith(".amdhsa_kernel"):
            part = 1
        elif s.startswith(".end_amdhsa_kernel"):
            part = None
        elif s.startswith(".section") or s.startswith(".p2align") or s == ".text":
            part = None if part == 0 else part
        elif s and part is not None:
            out[sym][part].append(re.sub(r"\.(LBB|Lfunc_end|LJTI)\d+", r".\1", s))
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for sym in sorted(set(a) | set(b)):
        if sym not in a or sym not in b:
            verdict = "only in " + (sys.argv[1] if sym in a else sys.argv[2])
        elif a[sym][0] != b[sym][0]:
            verdict = "INSTRUCTIONS DIFFER (%d / %d lines)" % (len(a[sym][0]), len(b[sym][0]))
        elif a[sym][1] != b[sym][1]:
            verdict = "DESCRIPTOR DIFFERS: " + "; ".join(
                "%s -> %s" % (x, y) for x, y in zip(a[sym][1], b[sym][1]) if x != y)
        else:
            verdict = "same: %d instruction lines, %d descriptor lines" % (len(a[sym][0]), len(a[sym][1]))
        bad += not verdict.startswith("same")
        print("%s  %s" % (sym, verdict))
    nb = sum(s.startswith(HOT[0]) for s in b)
    print("%d k_body and %d k_constraint instantiations compared, %d differ" % (nb, len(b) - nb, bad))
    sys.exit(1 if bad or not b else 0)


if __name__ == "__main__":
    main()
