"""Per-kernel comparison of two hipcc device listings (``-S --cuda-device-only``) of one translation unit.

    python tools/compare_listings.py PARENT.s NEW.s

Prints, per kernel: whether its body is identical, and vgpr_count / vgpr_spill_count / private_segment_fixed_size /
group_segment_fixed_size (from the metadata) and the instruction count (from the body), parent -> new.  Lines with .file, .ident or
__hip_cuid are dropped first.  Exit status 1 when a kernel whose body changed misses the bounds of the policy fold (profiles/policy_fold_listings.txt):
VGPRs not above the parent's, no spills, no scratch, LDS equal, instruction count within 1 %.
"""
import re
import sys

KEYS = ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


def read(path):
    lines = [l.rstrip("\n") for l in open(path) if not any(w in l for w in (".file", ".ident", "__hip_cuid"))]
    bodies, name = {}, None
    for l in lines:
        m = re.match(r"^(_Z\w+):", l)
        if m and name is None:
            name = m.group(1)
            bodies[name] = []
        elif name is not None:
            if l.startswith(".Lfunc_end"):
                name = None
            else:
                l = re.sub(r"\.L(BB|tmp|func_\w+?)\d+", r".L\1", l)    # (local label numbers follow the order of the functions,
                l = re.sub(r"\bBB\d+_(\d+)", r"BB_\1", l)                # also where a loop comment names a block: Header=BB4_8,
                bodies[name].append(re.sub(r"\s+;", " ;", l))                # and the comment column moves with the label's width)
    meta, cur = {}, None
    for l in lines:
        m = re.match(r"^\s+(?:- )?\.(\w+):\s+(\S+)$", l)
        if not m:
            continue
        if l.lstrip().startswith("- ") and m.group(1) != "name":
            cur = {}                                   # a new kernel record starts with its first key
        if cur is None:
            continue
        cur[m.group(1)] = m.group(2)
        if m.group(1) == "name":
            meta[m.group(2)] = cur
    return lines, bodies, meta


def n_instr(body):
    return sum(1 for l in body if re.match(r"^\t[a-z]", l))


def main(a, b):
    la, ba, ma = read(a)
    lb, bb, mb = read(b)
    print("whole listing: %s (%d / %d lines)" % ("IDENTICAL" if la == lb else "differs", len(la), len(lb)))
    bad = 0
    kernels = [k for k in ma if k in ba]
    if set(ma) != set(mb):
        print("kernel sets differ:", sorted(set(ma) ^ set(mb)))
        bad += 1
    print("%-9s %-13s %-9s %-9s %-11s %-15s  kernel" % ("body", "vgpr", "spill", "scratch", "lds", "instructions"))
    for k in [k for k in mb if k not in ma and k in bb]:      # only in the new listing: no parent to stay below, the absolute bounds hold
        vb = [int(mb[k][x]) for x in KEYS]
        ok = vb[1] == 0 and vb[2] == 0
        bad += not ok
        print("%-9s %-13s %-9s %-9s %-11s %-15s  %s%s" % ("new", "-> %d" % vb[0], "-> %d" % vb[1], "-> %d" % vb[2], "-> %d" % vb[3], "-> %d" % n_instr(bb[k]), k,
                                                      "" if ok else "   <-- OUTSIDE THE BOUNDS"))
    for k in kernels:
        if k not in mb:
            continue
        va, vb = [int(ma[k][x]) for x in KEYS], [int(mb[k][x]) for x in KEYS]
        ia, ib = n_instr(ba[k]), n_instr(bb[k])
        ok = ba[k] == bb[k] or (vb[0] <= va[0] and vb[1] == 0 and vb[2] == 0 and vb[3] == va[3] and abs(ib - ia) <= 0.01 * ia)
        bad += not ok
        print("%-9s %-13s %-9s %-9s %-11s %-15s  %s%s" % ("same" if ba[k] == bb[k] else "changed", "%d -> %d" % (va[0], vb[0]), "%d -> %d" % (va[1], vb[1]),
                                                      "%d -> %d" % (va[2], vb[2]), "%d -> %d" % (va[3], vb[3]),
                                                      "%d -> %d" % (ia, ib), k, "" if ok else "   <-- OUTSIDE THE BOUNDS"))
    print("%d kernels, %d outside the bounds" % (len(kernels), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
