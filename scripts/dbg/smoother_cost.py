"""What the FFBS smoother costs.  Writes profiles/smoother_cost.log (and prints it).  Nothing here is a pass condition.
  shapes   1 x 1024, 1 x 8192 and 512 x 1024 (filters x particles), T = 200, LG1D and UCSV3D
  columns  time of smc_smooth (device events on the handle's stream, second of two calls) and its launch count; picoseconds per pair
           evaluation, pairs = 2 n_x^2 (T - 1) n_theta; the time of the plain step-by-step filter of the same series (host clock
           around init + T - 1 steps ending in a synchronise, second of two runs); the issue bound over the measured time
  bound    vector instructions per pair evaluation over 256 CUs x 64 f64 lanes per clock at the 2.4 GHz peak clock (the chip runs
           below it under load, so 100 % is not reachable).  The counts come from the ISA listing, per chunk length:
               python scripts/dbg/smoother_cost.py --isa        (needs hipcc, no GPU; writes profiles/smoother_isa_counts.json)
           compiles csrc/smc_capi_smooth.hip to gfx950 assembly (as scripts/dbg/isa.sh does for the step kernels), finds in every
           k_smooth_pairs<model, pass> the shortest backward-branch loop that reads LDS - the pair loop, unrolled 8 / 4 / 4 times
           in passes 0 / 1 / 2 - and counts its v_* instructions per pair.  A pair evaluation is (pass 0 + pass 1 + pass 2) / 2.
           The measuring run reads that file; without an entry for a chunk length the bound column says so.
  chunks   every candidate SMOOTH_CH (64, 128, 256): the product library is 128; the others are timing builds
           (make -C sequential_monte_carlo_amd/csrc smoothch CH=64) run in a child process each, with SMC_LIB set
Kernel statistics are a run of their own: rocprofv3 --kernel-trace --stats -- python scripts/dbg/smoother_cost.py --one 1x8192"""
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.environ.get("SMC_ROOT") or os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "sequential_monte_carlo_amd", "csrc")
COUNTS = os.path.join(ROOT, "profiles", "smoother_isa_counts.json")
LOG = os.path.join(ROOT, "profiles", "smoother_cost.log")
T = 200
SHAPES = ((1, 1024), (1, 8192), (512, 1024))
ROWS = {1: [0.5, 1.0, 0.9, 0.8, 0.0, 1.0], 3: [0.2, 0.2, 0.0, -1.0, -2.0]}
NAMES = {1: "LG1D", 3: "UCSV3D"}
UNROLL = (8, 4, 4)
LANES_PER_SECOND = 256 * 64 * 2.4e9


def isa_counts(ch):
    """{model: vector instructions per pair evaluation} of the build with SMOOTH_CH = ch, from the gfx950 listing"""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "smooth.s")
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                               "-fno-fast-math", "-fPIC", "-DSMC_SMOOTH_CH=%d" % ch, "--cuda-device-only", "-S", "-o", out,
                               os.path.join(CSRC, "smc_capi_smooth.hip")], stderr=subprocess.DEVNULL)
        text = open(out).read().split("\n")
    res = {}
    for model in (1, 3):
        per_pass = []
        for ps in range(3):
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
            per_pass.append(sum(1 for q in best if re.match(r"^\s+v_", q)) / UNROLL[ps])
        res[str(model)] = {"per_pass": per_pass, "per_pair_evaluation": sum(per_pass) / 2}
    return res


def run_steps(h, y):
    h.init(float(y[0]))
    for t in range(1, len(y)):
        h.step(float(y[t]))
    h.synchronize()


def measure(ch, shapes):
    import numpy as np
    from sequential_monte_carlo_amd import _lib as L
    counts = json.load(open(COUNTS)).get(str(ch)) if os.path.exists(COUNTS) else None
    for model in (1, 3):
        _, y = L.simulate(model, ROWS[model], T, 1998)
        for nth, n in shapes:
            h = L.Handle(model, nth, n, seed=3)
            h.set_params(np.tile(ROWS[model], (nth, 1)))
            filt = []
            for _ in range(2):
                t0 = time.perf_counter()
                run_steps(h, y)
                filt.append((time.perf_counter() - t0) * 1e3)
            h.history_begin(T)
            run_steps(h, y)
            ms = []
            for _ in range(2):
                h.smooth(weights=False, moments=True)
                ms.append(h.elapsed_ms())
            h.close()
            pairs = 2.0 * n * n * (T - 1) * nth
            nchunk = (n + ch - 1) // ch
            launches = (6 if nchunk > 8 else 5) * (T - 1) + 3
            if counts:
                per = counts[str(model)]["per_pair_evaluation"]
                bound_ms = pairs * per / LANES_PER_SECOND * 1e3
                bound = "issue bound (%.1f instructions / pair evaluation) %8.3f ms = %4.1f %% of the time" % (per, bound_ms, 100 * bound_ms / ms[1])
            else:
                bound = "issue bound not computed (no ISA counts for this chunk length: --isa)"
            print("CH %3d  %-6s %3d x %-5d T %d: smooth %9.3f ms (first call %9.3f), %d launches, %7.2f ps / pair evaluation, %s; "
                  "step-by-step filter %8.3f ms" % (ch, NAMES[model], nth, n, T, ms[1], ms[0], launches, ms[1] * 1e9 / pairs, bound, filt[1]),
                  flush=True)


if __name__ == "__main__":
    if "--isa" in sys.argv:
        json.dump({str(ch): isa_counts(ch) for ch in (64, 128, 256)}, open(COUNTS, "w"), indent=1, sort_keys=True)
        print(open(COUNTS).read())
        sys.exit(0)
    if "--child" in sys.argv or "--one" in sys.argv:
        ch = int(os.environ.get("SMOOTH_COST_CH", "128"))
        shapes = SHAPES
        if "--one" in sys.argv:
            a, b = sys.argv[sys.argv.index("--one") + 1].split("x")
            shapes = ((int(a), int(b)),)
        measure(ch, shapes)
        sys.exit(0)
    lines = []
    for ch in (64, 128, 256):
        env = dict(os.environ, SMOOTH_COST_CH=str(ch))
        if ch != 128:
            lib = os.path.join(CSRC, "build_ch%d" % ch, "libsmchip_ch%d.so" % ch)
            if not os.path.exists(lib):
                lines.append("CH %3d  not measured: %s is not built (make -C %s smoothch CH=%d)" % (ch, os.path.relpath(lib, ROOT), os.path.relpath(CSRC, ROOT), ch))
                print(lines[-1], flush=True)
                continue
            env["SMC_LIB"] = lib
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, stdout=subprocess.PIPE, text=True)
        print(r.stdout, end="", flush=True)
        lines += r.stdout.splitlines()
        if r.returncode != 0:       # a child that failed may have left the device in trouble: start nothing more on it
            print("CH %3d  the measurement ended with status %d; stopping" % (ch, r.returncode), flush=True)
            sys.exit(r.returncode)
    with open(LOG, "w") as f:
        f.write("\n".join(lines) + "\n")
