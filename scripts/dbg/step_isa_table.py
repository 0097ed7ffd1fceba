"""Diagnostic (no GPU): registers of every k_step* instantiation in two assembly dumps of smc_model.hip (parent, candidate), and the
f64 instructions inside the LDS ancestor search of one instantiation, and how many bodies are the parent's instruction for
instruction.  The dumps are those of `make -C sequential_monte_carlo_amd/csrc isa` in a checkout of each commit
(build_isa/plain.<model>.s: the Makefile's flags and preload count, --cuda-device-only -S).
usage: step_isa_table.py <parent.s> <candidate.s> [mangled prefix of the kernel whose search is counted]"""
import re
import sys

FLAG = "_ZN3smc6k_stepILi1ELi512ELi2ELb1ELb0ELb0ELi1ELb0ELb1EE"


def kernels(path):
    """{name: (lines of the body, {NumVgprs, Occupancy, ScratchSize})} of the k_step* kernels"""
    out, name, body, meta = {}, None, [], None
    for line in open(path):
        m = re.match(r"^(_ZN3smc6k_step\w+):", line)
        if m:
            name, body, meta = m.group(1), [], {}
            continue
        if name is None:
            continue
        if body is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = [body, meta]
                body = None
            else:
                body.append(line)
            continue
        m = re.match(r"^; (NumVgprs|Occupancy|ScratchSize): (\d+)", line)
        if m:
            meta[m.group(1)] = int(m.group(2))
            if len(meta) == 3:
                name = None
    return out


def normal(body):
    """the instructions of a body without comments, with the block labels (numbered per function of the file) made anonymous"""
    out = []
    for l in body:
        l = re.sub(r"\.L\w+", ".L", l.split(";")[0]).strip()
        if l:
            out.append(l)
    return out


def search_f64(body):
    """(LDS reads, VALU, f64 instructions) between the first and the last ds_read_b64 of the search: behind the last `s_setprio 1`
    (the staging barrier) and ahead of the first gather (`; collapsed or ragged`)"""
    lo = max(i for i, l in enumerate(body) if "s_setprio 1" in l)
    hi = min(i for i, l in enumerate(body) if i > lo and "collapsed or ragged" in l)
    reads = [i for i in range(lo, hi) if "ds_read_b64" in body[i]]
    seg = body[reads[0]:reads[-1] + 1]
    valu = [l for l in seg if re.match(r"^\s+v_", l)]
    return len(reads), len(valu), sum(1 for l in valu if re.match(r"^\s+v_\w*f64", l))


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    flag = sys.argv[3] if len(sys.argv) > 3 else FLAG
    print("# %s -> %s" % (sys.argv[1].split("/")[-1], sys.argv[2].split("/")[-1]))
    print("# kernel  NumVgprs  Occupancy  ScratchSize   (parent -> candidate; * = changed, ! = occupancy lost or scratch gained)")
    worse = 0
    for k in sorted(a):
        p, c = a[k][1], b[k][1]
        bad = c["Occupancy"] < p["Occupancy"] or c["ScratchSize"] > p["ScratchSize"]
        worse += bad
        mark = "!" if bad else "*" if p != c else " "
        print("%s %s  %d -> %d  %d -> %d  %d -> %d" % (mark, k, p["NumVgprs"], c["NumVgprs"], p["Occupancy"], c["Occupancy"], p["ScratchSize"], c["ScratchSize"]))
    print("# %d instantiations, %d lost occupancy or gained scratch; kernels only in one dump: %s" % (len(a), worse, sorted(set(a) ^ set(b))))
    print("# %d bodies are the parent's instruction for instruction" % sum(1 for k in a if k in b and normal(a[k][0]) == normal(b[k][0])))
    for tag, d in (("parent", a), ("candidate", b)):
        ks = [k for k in d if k.startswith(flag)]
        if ks:
            print("# search of %s, %s: %d ds_read_b64, %d VALU, %d f64 instructions between the first and the last read" % ((ks[0][:60], tag) + search_f64(d[ks[0]][0])))


if __name__ == "__main__":
    main()
