"""What backward simulation costs.  Writes profiles/paths_cost.log (and prints it).  Nothing here is a pass condition.
  shapes   1 x 1024, 1 x 8192 and 512 x 1024 (filters x particles), T = 200, LG1D and UCSV3D; M = n_x paths for the lone filters,
           M = 16 and M = 1024 for the batch
  columns  time of smc_sample_paths (device events on the handle's stream, second of two calls; no output copied) and its launch
           count; picoseconds per pair evaluation, pairs = 2 M n_x T n_theta (passes A and B at every recorded step, the last one
           included); smc_smooth on the SAME record in the same session (second of two calls) and the ratio of the two times; the
           issue bound over the measured time
  bound    vector instructions per pair evaluation over 256 CUs x 64 f64 lanes per clock at the 2.4 GHz peak clock, as
           scripts/dbg/smoother_cost.py states it for the smoother.  The counts come from the ISA listing:
               python scripts/dbg/paths_cost.py --isa        (needs hipcc, no GPU; writes profiles/paths_isa_counts.json)
           finds in every k_path_pairs<model, pass> the shortest backward-branch loop that reads LDS - the pair loop, unrolled
           8 / 4 times in passes A / B - and counts its v_* instructions per pair; a pair evaluation is (pass A + pass B) / 2.
           k_path_select (one chunk recomputed per path, M SMOOTH_CH evaluations per step with per-lane gathers) is not in the bound.
  select   k_path_select has two shapes (one wave per path below PATH_WAVE_SELECT = 262144 paths, one thread per path from there
           on; the same indices).  The log holds three blocks, each a child process of its own: the product library, and the two
           timing builds that force one shape at every size (never shipped; loaded with SMC_LIB):
               make -C sequential_monte_carlo_amd/csrc pathsel SEL=0                        one thread per path
               make -C sequential_monte_carlo_amd/csrc pathsel SEL=4611686018427387904      one wave per path
           Besides the shapes above every block runs a sweep of n_theta x 1024 particles with M = 1024 paths, n_theta = 16, 32, 64,
           128 and 256 (16384 .. 262144 paths): what the threshold rests on."""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.environ.get("SMC_ROOT") or os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "sequential_monte_carlo_amd", "csrc")
COUNTS = os.path.join(ROOT, "profiles", "paths_isa_counts.json")
LOG = os.path.join(ROOT, "profiles", "paths_cost.log")
T = 200
SHAPES = ((1, 1024, 1024), (1, 8192, 8192), (512, 1024, 16), (512, 1024, 1024))     # (filters, particles, paths)
SWEEP = ((16, 1024, 1024), (32, 1024, 1024), (64, 1024, 1024), (128, 1024, 1024), (256, 1024, 1024))
VARIANTS = (("library", None, "the product library: one wave per path below n_theta M = 262144 paths, one thread per path from there on"),
            ("thread", "0", "timing build, k_path_select with ONE THREAD per path at every size"),
            ("wave", "4611686018427387904", "timing build, k_path_select with ONE WAVE per path at every size"))
ROWS = {1: [0.5, 1.0, 0.9, 0.8, 0.0, 1.0], 3: [0.2, 0.2, 0.0, -1.0, -2.0]}
NAMES = {1: "LG1D", 3: "UCSV3D"}
UNROLL = (8, 4)
LANES_PER_SECOND = 256 * 64 * 2.4e9


def isa_counts():
    """{model: vector instructions per pair evaluation} from the gfx950 listing"""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "smooth.s")
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                               "-fno-fast-math", "-fPIC", "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "smc_capi_smooth.hip")],
                              stderr=subprocess.DEVNULL)
        text = open(out).read().split("\n")
    res = {}
    for model in (1, 3):
        per_pass = []
        for ps in range(2):
            name = "_ZN3smc12k_path_pairsILi%dELi%dEE" % (model, ps)
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


def measure(label):
    import numpy as np
    from sequential_monte_carlo_amd import _lib as L
    counts = json.load(open(COUNTS)) if os.path.exists(COUNTS) else None
    lines = []
    for model in (1, 3):
        _, y = L.simulate(model, ROWS[model], T, 1998)
        h, shape = None, None
        for nth, n, M in SHAPES + SWEEP:
            if shape != (nth, n):
                if h is not None:
                    h.close()
                h, shape = L.Handle(model, nth, n, seed=3), (nth, n)
                h.set_params(np.tile(ROWS[model], (nth, 1)))
                h.history_begin(T)
                run_steps(h, y)
                sm = []
                for _ in range(2):
                    h.smooth(weights=False, moments=False)
                    sm.append(h.elapsed_ms())
            ms = []
            for _ in range(2):
                L.check(L.lib().smc_sample_paths(h._h, M, 20260117, None, None, None))
                ms.append(h.elapsed_ms())
            pairs = 2.0 * M * n * T * nth
            nchunk = (n + L.SMOOTH_CH - 1) // L.SMOOTH_CH
            launches = (4 if nchunk > 8 else 3) * T + 1
            if counts:
                per = counts[str(model)]["per_pair_evaluation"]
                bound_ms = pairs * per / LANES_PER_SECOND * 1e3
                bound = "issue bound (%.1f instructions / pair evaluation) %8.3f ms = %4.1f %% of the time" % (per, bound_ms, 100 * bound_ms / ms[1])
            else:
                bound = "issue bound not computed (no ISA counts: --isa)"
            lines.append("%-7s %-6s %3d x %-5d M %-5d T %d: sample_paths %9.3f ms (first call %9.3f), %d launches, %7.2f ps / pair evaluation, %s; "
                         "smc_smooth on the same record %9.3f ms, paths / smooth = %.2f"
                         % (label, NAMES[model], nth, n, M, T, ms[1], ms[0], launches, ms[1] * 1e9 / pairs, bound, sm[1], ms[1] / sm[1]))
            print(lines[-1], flush=True)
        h.close()
    return lines


if __name__ == "__main__":
    if "--isa" in sys.argv:
        json.dump(isa_counts(), open(COUNTS, "w"), indent=1, sort_keys=True)
        print(open(COUNTS).read())
        sys.exit(0)
    if "--child" in sys.argv:
        measure(sys.argv[sys.argv.index("--child") + 1])
        sys.exit(0)
    lines = ["# scripts/dbg/paths_cost.py, one MI355X, one session, T = %d; smc_sample_paths by device events, second of two calls; "
             "smc_smooth on the same record" % T]
    for label, sel, what in VARIANTS:
        env = dict(os.environ)
        if sel is not None:
            lib = os.path.join(CSRC, "build_sel" + sel, "libsmchip_sel%s.so" % sel)
            if not os.path.exists(lib):
                lines.append("# %s: not measured, %s is not built (make -C %s pathsel SEL=%s)" % (label, os.path.relpath(lib, ROOT), os.path.relpath(CSRC, ROOT), sel))
                print(lines[-1], flush=True)
                continue
            env["SMC_LIB"] = lib
        lines.append("# %s: %s" % (label, what))
        print(lines[-1], flush=True)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", label], env=env, stdout=subprocess.PIPE, text=True)
        print(r.stdout, end="", flush=True)
        lines += r.stdout.splitlines()
        if r.returncode != 0:       # a child that failed may have left the device in trouble: start nothing more on it
            print("%s: the measurement ended with status %d; stopping" % (label, r.returncode), flush=True)
            sys.exit(r.returncode)
    with open(os.environ.get("PATHS_COST_LOG", LOG), "w") as f:
        f.write("\n".join(lines) + "\n")
