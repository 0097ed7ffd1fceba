"""What the lag-one pair moments cost.  Writes profiles/pairs_cost.log (and prints it).  Nothing here is a pass condition.
  shapes   1 x 1024, 1 x 8192 and 512 x 1024 (filters x particles), T = 200, LG1D and UCSV3D, one session
  columns  smc_smooth_pairs against smc_smooth on the same record, interleaved (smooth, pairs, smooth, pairs; device events on the
           handle's stream, the second call of each), and their ratio.  With --parent DIR the same shapes are run once more in a child
           process that imports the package of DIR (a built tree of the parent commit) and times its smc_smooth: the unflagged call
           did not move.
  variance N = 1024, T = 200, 64 filters of UCSV3D: the variance over the filters of sum_t resid2[t][lse] against the same statistic
           from 256 backward-simulated paths of the same records (the mean over the paths of sum_t (lse_{t+1} - lse_t)^2)
  --isa    (needs hipcc, no GPU; writes profiles/pairs_isa_counts.json) compiles csrc/smc_capi_smooth.hip to gfx950 assembly and
           counts the v_* instructions per pair in the pair loop of k_smooth_pairs<model, 2> and <model, 3>, as
           scripts/dbg/smoother_cost.py --isa does, with the registers, LDS and scratch of both from the listing's metadata"""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.environ.get("SMC_ROOT") or os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "sequential_monte_carlo_amd", "csrc")
COUNTS = os.path.join(ROOT, "profiles", "pairs_isa_counts.json")
LOG = os.path.join(ROOT, "profiles", "pairs_cost.log")
T = 200
SHAPES = ((1, 1024), (1, 8192), (512, 1024))
ROWS = {1: [0.5, 1.0, 0.9, 0.8, 0.0, 1.0], 3: [0.2, 0.2, 0.0, -1.0, -2.0]}
NAMES = {1: "LG1D", 3: "UCSV3D"}
UNROLL = 4


def isa_counts():
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "smooth.s")
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                               "-fno-fast-math", "-fPIC", "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "smc_capi_smooth.hip")],
                              stderr=subprocess.DEVNULL)
        text = open(out).read().split("\n")
    res = {}
    for model in (1, 3):
        for ps in (2, 3):
            name = "_ZN3smc14k_smooth_pairsILi%dELi%dEE" % (model, ps)
            start = next(i for i, l in enumerate(text) if re.match("^" + name + r"\w*:", l))
            end = next(i for i in range(start, len(text)) if text[i].startswith(".Lfunc_end"))
            body, labels, best = text[start:end], {}, None
            for i, l in enumerate(body):
                m = re.match(r"^(\.LBB\d+_\d+):", l)
                if m:
                    labels[m.group(1)] = i
                m = re.search(r"s_cbranch_\w+\s+(\.LBB\d+_\d+)", l)
                if m and m.group(1) in labels:
                    loop = body[labels[m.group(1)]:i + 1]
                    if any("ds_read" in q for q in loop) and (best is None or len(loop) < len(best)):
                        best = loop
            meta = {}
            for l in text[end:end + 80]:
                m = re.match(r"^; (NumVgprs|NumSgprs|ScratchSize|LDSByteSize|Occupancy): (\d+)", l)
                if m and m.group(1) not in meta:
                    meta[m.group(1)] = int(m.group(2))
            res["%s pass %d" % (NAMES[model], ps)] = dict(meta, valu_per_pair=sum(1 for q in best if re.match(r"^\s+v_", q)) / UNROLL,
                                                          lds_reads_per_pair=sum(1 for q in best if "ds_read" in q) / UNROLL)
    return res


def record(L, np, model, nth, n):
    _, y = L.simulate(model, ROWS[model], T, 1998)
    h = L.Handle(model, nth, n, seed=3)
    h.set_params(np.tile(ROWS[model], (nth, 1)))
    h.history_begin(T)
    h.init(float(y[0]))
    for t in range(1, T):
        h.step(float(y[t]))
    return h


def measure(parent):
    import numpy as np
    from sequential_monte_carlo_amd import _lib as L
    for model in (1, 3):
        for nth, n in SHAPES:
            h = record(L, np, model, nth, n)
            ms = {False: [], True: []}
            for _ in range(2):
                for pairs in ((False,) if parent else (False, True)):
                    h.smooth(weights=False, moments=True, **({"pairs": True} if pairs else {}))
                    ms[pairs].append(h.elapsed_ms())
            h.close()
            if parent:
                print("parent  %-6s %3d x %-5d T %d: smc_smooth %9.3f ms" % (NAMES[model], nth, n, T, ms[False][1]), flush=True)
            else:
                print("%-6s %3d x %-5d T %d: smc_smooth %9.3f ms, smc_smooth_pairs %9.3f ms, ratio %.3f" % (
                    NAMES[model], nth, n, T, ms[False][1], ms[True][1], ms[True][1] / ms[False][1]), flush=True)
    if parent:
        return
    # what the feature buys: the spread of the UCSV E-step statistic over independent filters, pairs against 256 paths
    nth, n, M = 64, 1024, 256
    h = record(L, np, 3, nth, n)
    resid2 = h.smooth(weights=False, pairs=True)[4]                     # [T-1][3][nth]
    _, xs = h.sample_paths(M, 17)                                       # [T][3][nth][M]
    h.close()
    a = resid2[:, 1, :].sum(axis=0)
    b = (np.diff(xs[:, 1], axis=0) ** 2).sum(axis=0).mean(axis=1)
    print("UCSV3D %d x %d T %d, sum_t resid2[t][lse] over the filters: pairs mean %.5f variance %.3e; %d paths mean %.5f variance %.3e; "
          "variance of the difference %.3e" % (nth, n, T, a.mean(), a.var(ddof=1), M, b.mean(), b.var(ddof=1), (b - a).var(ddof=1)), flush=True)


if __name__ == "__main__":
    if "--isa" in sys.argv:
        json.dump(isa_counts(), open(COUNTS, "w"), indent=1, sort_keys=True)
        print(open(COUNTS).read())
        sys.exit(0)
    if "--child" in sys.argv:
        measure(parent="--as-parent" in sys.argv)
        sys.exit(0)
    lines = []
    runs = [(dict(os.environ), [])]
    if "--parent" in sys.argv:      # the tree of the parent commit, built: the child imports ITS package (SMC_ROOT) and so loads its library
        runs.append((dict(os.environ, SMC_ROOT=os.path.abspath(sys.argv[sys.argv.index("--parent") + 1])), ["--as-parent"]))
    for env, extra in runs:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + extra, env=env, stdout=subprocess.PIPE, text=True)
        print(r.stdout, end="", flush=True)
        lines += r.stdout.splitlines()
        if r.returncode != 0:       # a child that failed may have left the device in trouble: start nothing more on it
            print("the measurement ended with status %d; stopping" % r.returncode, flush=True)
            sys.exit(r.returncode)
    with open(LOG, "w") as f:
        f.write("\n".join(lines) + "\n")
