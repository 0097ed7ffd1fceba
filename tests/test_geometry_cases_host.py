"""tests/geometry_cases.py against the sources it mirrors, and the coverage of the cases it generates (no GPU, no library).

  a. the mirror: the cases of SMC_GEO_SWITCH, geo_default, the enumerations, LAUNCH_FAMILIES and LAUNCH_OBJECT, STEP_BYV / STEP_SYS,
     the geometry tables of the resident and window launchers, the rule of resident_np and the Makefile's KERNELS, by regular
     expression (as test_host.py::test_julia_binding_matches_header reads the header): a geometry, a (variant, family) pair or an
     entry added to the sources without a case fails here
  b. the arithmetic of every case: nseg, nseg_p2 and the shape recomputed from (n, seg, threads)
  c. the coverage conditions
  d. the exclusions: shapes M2 and G at 512 threads and more only, listed with their reason; no triple left out altogether
"""
import collections
import os
import re

import geometry_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sequential_monte_carlo_amd", "csrc")
MODEL_IDS = {"MODEL_LG1D": 1, "MODEL_SV1D": 2, "MODEL_UCSV3D": 3, "MODEL_UCSV_RB": 4}


def read(name):
    return open(os.path.join(CSRC, name)).read()


def enum_names(src, name):
    body = re.search(r"enum %s : int \{(.*?)\};" % name, src, flags=re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    return [w.split("=")[0].strip() for w in body.split(",") if w.strip()]


def variant_names(launch):
    names = enum_names(launch, "Variant")
    assert names[-1] == "VARIANT_COUNT"
    return [n[len("VARIANT_"):].lower() for n in names[:-1]]


# ---- a. the mirror ------------------------------------------------------------------------------------------------------------------
def test_geometries_are_the_cases_of_the_switch():
    model = read("smc_model.hip")
    macro = re.search(r"#define SMC_GEO_SWITCH\(FN, \.\.\.\)(.*?)\n\n", model, flags=re.S).group(1)
    cases = re.findall(r"case (\d+) \* 8 \+ (\d+): return FN<(\d+), (\d+)>", macro)
    assert len(cases) == macro.count("case ") and all(c[:2] == c[2:] for c in cases)
    assert sorted((int(a), int(b)) for a, b, _, _ in cases) == sorted(GC.GEOMETRIES) and len(set(GC.GEOMETRIES)) == 13
    # what geo_valid accepts, evaluated from its text: np in {1, 2, 4}, threads = seg / (2 np) one of the listed ones
    capi = read("smc_capi.hip")
    body = re.search(r"bool geo_valid\(int seg, int np, Geo& g\) \{(.*?)\n\}", capi, flags=re.S).group(1)
    assert "np != 1 && np != 2 && np != 4" in body
    cond = re.search(r"if \(!\((th == .*?)\)\) return false;", body).group(1)
    ok = lambda th, np: eval(cond.replace("&&", " and ").replace("||", " or "), {"th": th, "np": np})   # noqa: E731
    accepted = {(seg // (2 * k), k) for seg in (256, 512, 1024, 2048, 4096, 8192) for k in (1, 2, 4) if ok(seg // (2 * k), k)}
    assert accepted == set(GC.GEOMETRIES)
    defaults = re.findall(r"case (\d+): g = \{(\d+), (\d+)\}; return true;", capi)
    assert {int(s): (int(t), int(k)) for s, t, k in defaults} == GC.DEFAULT
    assert all(g in GC.GEOMETRIES and GC.seg_of(*g) == s for s, g in GC.DEFAULT.items())


def test_variants_families_and_entries():
    launch = read("smc_launch.h")
    names = variant_names(launch)
    assert tuple(names) == GC.VARIANTS
    entries = enum_names(launch, "Entry")
    assert entries[-1] == "ENTRY_COUNT" and tuple(e[len("ENTRY_"):].lower() for e in entries[:-1]) == GC.ENTRIES
    fam = re.search(r"LAUNCH_FAMILIES\[VARIANT_COUNT\] = \{(.*?)\};", launch, flags=re.S).group(1)
    rows = re.findall(r"family_bits\(([^)]*)\)", fam)
    assert len(rows) == len(names)
    for name, row in zip(names, rows):
        assert tuple(MODEL_IDS[m.strip()] for m in row.split(",")) == GC.FAMILIES[name], name
    obj = re.search(r"LAUNCH_OBJECT\[VARIANT_COUNT\]\[ENTRY_COUNT\] = \{(.*?)\n\};", launch, flags=re.S).group(1)
    rows = re.findall(r"\*/ \{([^}]*)\}", obj)
    assert len(rows) == len(names)
    for name, row in zip(names, rows):
        cells = tuple(None if c.strip() == "NO_OBJECT" else c.strip()[len("VARIANT_"):].lower() for c in row.split(","))
        assert cells == GC.LAUNCH_OBJECT[name], name


def test_objects_are_the_kernels_of_the_makefile():
    mk = read("Makefile").replace("\\\n", " ")
    kernels = re.search(r"^KERNELS = (.*)$", mk, flags=re.M).group(1).split()
    assert sorted(kernels) == sorted("%s.%d" % o for o in GC.OBJECTS) and len(kernels) == 15
    ids = {n: int(i) for n, i in re.findall(r"^VARIANT_(\w+) = (\d+)$", mk, flags=re.M)}
    assert ids == {n: k for k, n in enumerate(GC.VARIANTS)}


def test_step_byv_and_step_sys():
    """the constexpr flags of smc_model.hip evaluated from their text for every variant id"""
    model = read("smc_model.hip")
    exprs = dict(re.findall(r"constexpr bool (VAR_GUIDED|VAR_MISS|VAR_COND|STEP_BYV|STEP_SYS) = ([^;]*);", model))
    assert len(exprs) == 5
    for k, name in enumerate(GC.VARIANTS):
        env = {"VAR": k}
        env.update({"VARIANT_" + n.upper(): j for j, n in enumerate(GC.VARIANTS)})
        for flag in ("VAR_GUIDED", "VAR_MISS", "VAR_COND", "STEP_BYV", "STEP_SYS"):
            env[flag] = bool(eval(exprs[flag].replace("&&", " and ").replace("||", " or ").replace("!", " not "), dict(env)))
        assert env["STEP_BYV"] == GC.STEP_BYV[name] and env["STEP_SYS"] == GC.STEP_SYS[name], name
    capi = read("smc_capi.hip")
    assert re.search(r"n_x > PATH_MAX_N\) return fail\(SMC_EINVAL, \"smc_create: SMC_FLAG_CONDITIONAL with n_x > 2\^20", capi)
    assert "constexpr int64_t PATH_MAX_N = (int64_t)1 << 20;" in read("smc_spec.h")
    assert GC.COND_MAX_N == 1 << 20
    # ... and the table shapes a conditional handle can never reach are not instantiated: exactly the UNREACHABLE cells
    has = dict(re.findall(r"constexpr bool (HAS_GTAB|HAS_RPT2) = !VAR_COND \|\| ([^;]*);", model))
    assert has == {"HAS_GTAB": "2 * THREADS * SEG < PATH_MAX_N", "HAS_RPT2": "THREADS * SEG < PATH_MAX_N"}
    assert "constexpr int64_t SEG = 2 * NP * THREADS;" in model
    for th, k in GC.GEOMETRIES:
        env = {"THREADS": th, "SEG": 2 * k * th, "PATH_MAX_N": GC.COND_MAX_N}
        for shape, flag in (("M2", "HAS_RPT2"), ("G", "HAS_GTAB")):
            assert eval(has[flag], dict(env)) == (not GC.unreachable("cond", th, k, shape)), (th, k, shape)
            assert not GC.unreachable("plain", th, k, shape) and not GC.unreachable("cond", th, k, "M1")


def test_resident_tables():
    model = read("smc_model.hip")
    for entry, fn, window in (("resident", "resident_t", False), ("window", "window_t", True)):
        body = re.search(r"Launch<MODEL, VARIANT>::%s\(.*?\n\}" % entry, model, flags=re.S).group(0)
        blocks = re.split(r"\n\s*case (\d+):", body)[1:]
        table = {int(seg): {(int(a), int(b)) for a, b in re.findall(fn + r"<(\d+), (\d+)>", txt)} for seg, txt in zip(blocks[::2], blocks[1::2])}
        assert sorted(table) == [256, 512, 1024, 2048, 4096, 8192]
        for seg, geos in table.items():
            assert geos == {GC.resident_geo(seg, r, window) for r in (0, 1, 2, 4)}, (entry, seg)
            assert all(GC.seg_of(*g) == seg and g in GC.GEOMETRIES for g in geos)
    launch = read("smc_launch.h")
    rule = re.search(r"inline int resident_np\(const FilterView& v\) \{(.*?)\n\}", launch, flags=re.S).group(1)
    assert 'getenv("SMC_RES_NP")' in rule and "(v.seg == 1024 && v.ntheta <= 512) ? 1 : 0" in rule
    assert "resident_np(" not in model.split("Launch<MODEL, VARIANT>::resident")[0]      # one statement of the rule
    assert [GC.resident_np_default(1024, 512), GC.resident_np_default(1024, 513), GC.resident_np_default(2048, 1)] == [1, 0, 0]
    res = read("smc_resident.h")
    assert "lds_padded_len(seg) * 8 * (1 + d) + 2048 <= 160 * 1024" in res
    for m, d in GC.DIM.items():
        for seg in (256, 512) + GC.RESIDENT_SEGS:
            assert GC.resident_fits(m, seg) == ((seg + (seg >> 4) + 8) * 8 * (1 + d) + 2048 <= 160 * 1024), (m, seg)


# ---- b. the arithmetic of every case -----------------------------------------------------------------------------------------------
CASES = GC.step_cases()


def test_every_case_is_the_shape_it_claims():
    assert len(set(CASES)) == len(CASES)
    for c in CASES:
        assert (c.threads, c.np) in GC.GEOMETRIES and c.seg == 2 * c.np * c.threads, c
        nseg = -(-c.n // c.seg)
        p2 = 1 << (nseg - 1).bit_length()
        want = {"S": nseg == 1 and c.no_resident and c.n % c.seg != 0,
                "M1": nseg == 3 and p2 <= c.threads and c.n % c.seg != 0,
                "M2": c.threads < p2 == 2 * c.threads,
                "G": p2 > 2 * c.threads}[c.shape]
        assert want, (c, nseg, p2)
        assert GC.shape_of(c.n, c.seg, c.threads, c.no_resident) == c.shape, c
        assert c.no_resident == (c.shape == "S")
        assert c.T == (4 if c.n <= 1 << 20 else 3 if c.n < 1 << 24 else 2) and (c.T > 2 or (c.threads, c.np, c.shape) == (1024, 4, "G")), c
        assert c.nth == (2 if c.mode in ("mn", "sys") else 1)
        assert c.variant != "cond" or c.n <= GC.COND_MAX_N, c
        assert (c.kind != GC.NONE) == (c.variant in ("guided", "missing_guided")) and (c.kind != GC.AFFINE or c.model == GC.LG1D), c
        assert nseg <= 16384, c                                                  # MAX_NSEG of smc_create


# ---- c. coverage --------------------------------------------------------------------------------------------------------------------
def cells():
    out = collections.defaultdict(set)
    for c in CASES:
        out[(c.variant, c.model, c.threads, c.np)].add((c.shape, c.mode))
    return out


def test_coverage_conditions():
    launch_triples = {(v, m, th, k) for v in GC.VARIANTS for m in GC.FAMILIES[v] if GC.defines(v, "step") for th, k in GC.GEOMETRIES}
    assert launch_triples == set(GC.STEP_TRIPLES) and len(launch_triples) == 13 * 13
    got = cells()
    for t in GC.STEP_TRIPLES:
        v, m, th, k = t
        for shape in ("S", "M1"):
            assert (shape, "mn") in got[t], t
            if GC.STEP_SYS[v]:
                assert (shape, "sys") in got[t], t
            if GC.STEP_BYV[v]:
                assert (shape, "byv") in got[t], t
        if th <= 256:
            for shape in ("M2", "G"):
                assert (shape, "one") in got[t] or (v, m, th, k, shape) in GC.UNREACHABLE, (t, shape)
    # a flagged handle with a proposal (no step kernel of its own): both of the objects it launches, in S and M1
    for m in GC.FAMILIES["missing_guided"]:
        for th, k in GC.GEOMETRIES:
            assert {("S", "mn"), ("S", "sys"), ("M1", "mn"), ("M1", "sys")} <= got[("missing_guided", m, th, k)]


# ---- d. exclusions ------------------------------------------------------------------------------------------------------------------
def test_exclusions_are_limited_and_listed():
    got = cells()
    listed = {e[:5] for e in GC.EXCLUSIONS}
    assert len(listed) == len(GC.EXCLUSIONS)
    for v, m, th, k, shape, reason in GC.EXCLUSIONS:
        assert shape in ("M2", "G") and th >= 512 and reason.startswith("oracle cost"), (v, m, th, k, shape)
    # the only unreachable cells: a conditional handle above 2^20 particles, where even the smallest size of the shape is refused
    for v, m, th, k, shape in GC.UNREACHABLE:
        assert v == "cond" and shape in ("M2", "G") and {"M2": th, "G": 2 * th}[shape] * GC.seg_of(th, k) + 1 > GC.COND_MAX_N
    for t in GC.STEP_TRIPLES:
        for shape in GC.SHAPES:
            have = any(s == shape for s, _ in got[t])
            cell = t + (shape,)
            assert have != (cell in listed or cell in GC.UNREACHABLE), cell       # every cell is a case, or listed: never both, never neither
        assert any(s in ("S", "M1") for s, _ in got[t]), t                        # no triple is left out altogether
    # at 512 threads: every plain family and one family of each other variant; at 1024: LG1D and UCSV3D plain in M2, LG1D plain in G
    for th, k in ((512, 1), (512, 2), (512, 4)):
        for shape in ("M2", "G"):
            kept = {(v, m) for (v, m, a, b), s in got.items() if (a, b) == (th, k) and (shape, "one") in s}
            reach = {(v, m) for v, m in GC.KEEP_512 if (v, m, th, k, shape) not in GC.UNREACHABLE}
            assert kept == reach and {("plain", m) for m in (1, 2, 3, 4)} <= kept and {"guided", "missing"} <= {v for v, _ in kept}
    for th, k in ((1024, 1), (1024, 2), (1024, 4)):
        assert {(v, m) for (v, m, a, b), s in got.items() if (a, b) == (th, k) and ("M2", "one") in s} == {("plain", 1), ("plain", 3)}
        assert {(v, m) for (v, m, a, b), s in got.items() if (a, b) == (th, k) and ("G", "one") in s} == {("plain", 1)}
    big = [c for c in CASES if (c.threads, c.np, c.shape) == (1024, 4, "G")]
    assert len(big) == 1 and big[0].T == 2 and big[0].n == 2 * 1024 * 8192 + 7


def test_counts_per_object():
    per = GC.cases_per_object()
    assert set(per) == set(GC.OBJECTS)
    assert sum(per.values()) == len(CASES)
