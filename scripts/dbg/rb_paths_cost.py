"""What Rao-Blackwellised backward simulation costs and what it buys.  Writes profiles/rb_paths_cost.log (and prints it).  Nothing
here is a pass condition.
  shapes   those of profiles/paths_cost.log: 1 x 1024, 1 x 8192 and 512 x 1024 (filters x particles), T = 200; M = n_x paths for the
           lone filters, M = 16 and M = 1024 for the batch.  The marginal filter (MODEL_UCSV_RB) and bootstrap UCSV3D on the same
           series in the same session
  columns  time of smc_rb_sample_paths (walk, trend pass and summary; device events on the handle's stream, second of two calls;
           only the summary is copied) against smc_sample_paths of UCSV3D (second of two calls, nothing copied), their ratio, and
           picoseconds per pair evaluation, pairs = 2 M n_x T n_theta
  isa      vector instructions per pair evaluation of k_path_pairs<UCSV_RB> and k_path_pairs<UCSV3D> from the gfx950 listing, as
           scripts/dbg/paths_cost.py --isa counts them (the shortest backward-branch loop that reads LDS, per pair, passes A and B
           averaged):   python scripts/dbg/rb_paths_cost.py --isa     (needs hipcc, no GPU; writes profiles/rb_paths_isa_counts.json)
           The log and the division per pair are the expected extra.
  variance what the feature buys: the variance over K independent filters of the smoothed trend mean at every t, rb_smoother on
           MarginalUCSV against smoother(..., paths=M) on UCSV (the mean of the drawn trend paths) at equal N and M, and the ratio
           of the two averaged over t - reported whatever it is."""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.environ.get("SMC_ROOT") or os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "sequential_monte_carlo_amd", "csrc")
COUNTS = os.path.join(ROOT, "profiles", "rb_paths_isa_counts.json")
LOG = os.path.join(ROOT, "profiles", "rb_paths_cost.log")
T = 200
SHAPES = ((1, 1024, 1024), (1, 8192, 8192), (512, 1024, 16), (512, 1024, 1024))     # (filters, particles, paths)
ROW = [0.2, 0.2, 0.0, -1.0, -2.0]
UNROLL = (8, 4)
VAR_K, VAR_N, VAR_M, VAR_T = 64, 1024, 256, 50


def isa_counts():
    """{model: vector instructions per pair evaluation} from the gfx950 listing (the method of paths_cost.py)"""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "smooth.s")
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                               "-fno-fast-math", "-fPIC", "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "smc_capi_smooth.hip")],
                              stderr=subprocess.DEVNULL)
        text = open(out).read().split("\n")
    res = {}
    for model in (3, 4):
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


def recorded(L, np, model, nth, n, y):
    h = L.Handle(model, nth, n, seed=3)
    h.set_params(np.tile(ROW, (nth, 1)))
    h.history_begin(len(y))
    h.init(float(y[0]))
    for t in range(1, len(y)):
        h.step(float(y[t]))
    h.synchronize()
    return h


def measure():
    import numpy as np
    import sequential_monte_carlo_amd as smc
    from sequential_monte_carlo_amd import _lib as L
    lines = []
    if os.path.exists(COUNTS):
        c = json.load(open(COUNTS))
        lines.append("# vector instructions per pair evaluation (passes A, B; their mean): UCSV_RB %s, %.1f; UCSV3D %s, %.1f; extra %.1f"
                     % (c["4"]["per_pass"], c["4"]["per_pair_evaluation"], c["3"]["per_pass"], c["3"]["per_pair_evaluation"],
                        c["4"]["per_pair_evaluation"] - c["3"]["per_pair_evaluation"]))
    else:
        lines.append("# no ISA counts (--isa)")
    print(lines[-1], flush=True)
    _, y = L.simulate(3, ROW, T, 1998)
    for nth, n, M in SHAPES:
        ms = {}
        for model in (L.MODEL_UCSV_RB, 3):
            h = recorded(L, np, model, nth, n, y)
            t = []
            for _ in range(2):
                if model == 3:
                    L.check(L.lib().smc_sample_paths(h._h, M, 20260117, None, None, None))
                else:
                    h.rb_sample_paths(y, M, 20260117, per_path=False, summary=True)
                t.append(h.elapsed_ms())
            ms[model] = t
            h.close()
        pairs = 2.0 * M * n * T * nth
        rb, uc = ms[L.MODEL_UCSV_RB], ms[3]
        lines.append("%3d x %-5d M %-5d T %d: rb_sample_paths %9.3f ms (first call %9.3f), %7.2f ps / pair evaluation; sample_paths of UCSV3D "
                     "%9.3f ms (first call %9.3f), %7.2f ps / pair evaluation; rb / ucsv3d = %.2f"
                     % (nth, n, M, T, rb[1], rb[0], rb[1] * 1e9 / pairs, uc[1], uc[0], uc[1] * 1e9 / pairs, rb[1] / uc[1]))
        print(lines[-1], flush=True)
    # what it buys: K independent filters in one batch (filter k draws on stream k)
    yv = y[:VAR_T]
    _, _, _, sr = smc.rb_smoother(VAR_N, yv, [smc.MarginalUCSV((ROW[0], ROW[1]), ROW[2], (ROW[3], ROW[4]))] * VAR_K, paths=VAR_M, seed=7)
    _, _, _, su = smc.smoother(VAR_N, yv, [smc.UCSV((ROW[0], ROW[1]), ROW[2], (ROW[3], ROW[4]))] * VAR_K, paths=VAR_M, seed=7, smooth=False)
    vr = sr["trend_mean"].var(axis=1, ddof=1)                          # [T]
    vu = su["paths"][..., 0].mean(axis=2).var(axis=1, ddof=1)
    lines.append("variance over K = %d filters of the smoothed trend mean, N = %d, M = %d, T = %d: rb_smoother mean over t %.3e, smoother(paths) of UCSV "
                 "%.3e; ratio of the means %.3f, mean of the per-t ratios %.3f (min %.3f, max %.3f); difference of the two trend means, "
                 "largest |z| over t %.2f"
                 % (VAR_K, VAR_N, VAR_M, VAR_T, vr.mean(), vu.mean(), vr.mean() / vu.mean(), (vr / vu).mean(), (vr / vu).min(), (vr / vu).max(),
                    np.max(np.abs(sr["trend_mean"].mean(axis=1) - su["paths"][..., 0].mean(axis=2).mean(axis=1)) / np.sqrt((vr + vu) / VAR_K))))
    print(lines[-1], flush=True)
    return lines


if __name__ == "__main__":
    if "--isa" in sys.argv:
        json.dump(isa_counts(), open(COUNTS, "w"), indent=1, sort_keys=True)
        print(open(COUNTS).read())
        sys.exit(0)
    lines = ["# scripts/dbg/rb_paths_cost.py, one MI355X, one session, T = %d; device events, second of two calls" % T] + measure()
    with open(os.environ.get("RB_PATHS_COST_LOG", LOG), "w") as f:
        f.write("\n".join(lines) + "\n")
