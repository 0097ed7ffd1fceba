"""The case table of tests/test_gpu_geometry.py: every workgroup geometry (threads, np) of every kernel object, at the smallest
shapes that reach each segment-table form of the step kernel.  No GPU and no library here: tests/test_geometry_cases_host.py keeps
this mirror equal to the sources (SMC_GEO_SWITCH in smc_model.hip, LAUNCH_FAMILIES / LAUNCH_OBJECT in smc_launch.h, KERNELS in the
Makefile) and checks the arithmetic and the coverage of what step_cases() generates.

Shapes, for a geometry with seg = 2 np threads (nseg_p2: the segment count rounded up to a power of two):

  S   n = seg - 3, SMC_FLAG_NO_RESIDENT      one ragged segment, one k_step launch per step
  M1  n = 2 seg + 5                          three segments, one record per thread (MULTI, RPT = 1)
  M2  n = threads seg + 7                    nseg_p2 = 2 threads: two records per thread (RPT = 2)
  G   n = 2 threads seg + 7                  nseg_p2 = 4 threads: k_table and k_step<..., GTAB>

T = 4 (init and three steps: the resampler runs on non-uniform weights and reads the table of the step before), 3 above 2^20
particles, 2 for the one case of 2^24.
"""
import collections

# ---- the mirror ---------------------------------------------------------------------------------------------------------------------
# the cases of SMC_GEO_SWITCH (smc_model.hip) = what geo_valid (smc_capi.hip) accepts
GEOMETRIES = ((64, 2), (128, 1), (128, 2), (128, 4), (256, 1), (256, 2), (256, 4), (512, 1), (512, 2), (512, 4), (1024, 1), (1024, 2), (1024, 4))
# geo_default (smc_capi.hip)
DEFAULT = {256: (128, 1), 512: (256, 1), 1024: (512, 1), 2048: (512, 2), 4096: (1024, 2), 8192: (1024, 4)}
LG1D, SV1D, UCSV3D, UCSV_RB = 1, 2, 3, 4
DIM = {LG1D: 1, SV1D: 1, UCSV3D: 3, UCSV_RB: 4}
# enum Variant (smc_launch.h) = VARIANT_<name> of the Makefile
VARIANTS = ("plain", "guided", "missing", "missing_guided", "cond")
# LAUNCH_FAMILIES (smc_launch.h) = KERNELS (Makefile)
FAMILIES = {"plain": (1, 2, 3, 4), "guided": (1, 3), "missing": (1, 2, 3, 4), "missing_guided": (1, 3), "cond": (1, 2, 3)}
OBJECTS = tuple((v, m) for v in VARIANTS for m in FAMILIES[v])
# enum Entry and LAUNCH_OBJECT (smc_launch.h): the variant whose object serves each entry point of a variant, None = no such launch
ENTRIES = ("init", "step", "resident", "window", "forecast", "summ_once")
LAUNCH_OBJECT = {
    "plain": ("plain", "plain", "plain", "plain", "plain", "plain"),
    "guided": ("plain", "guided", "guided", "guided", None, None),
    "missing": ("missing", "missing", "missing", "missing", None, None),
    "missing_guided": ("missing", "missing", "missing_guided", "missing_guided", None, None),
    "cond": ("cond", "cond", None, None, None, None),
}
# STEP_BYV and STEP_SYS of smc_model.hip: the variants whose step kernels exist by value / with systematic resampling
STEP_BYV = {"plain": True, "guided": True, "missing": False, "missing_guided": False, "cond": False}
STEP_SYS = {"plain": True, "guided": True, "missing": True, "missing_guided": True, "cond": False}
# SMC_FLAG_CONDITIONAL is refused above 2^20 particles (smc_create: the limit of the backward walk)
COND_MAX_N = 1 << 20


def defines(variant, entry):
    """launch_defines (smc_launch.h)"""
    return LAUNCH_OBJECT[variant][ENTRIES.index(entry)] == variant


# the (variant, family, threads, np) triples that have a step kernel of their own
STEP_TRIPLES = tuple((v, m, th, k) for v, m in OBJECTS if defines(v, "step") for th, k in GEOMETRIES)

# ---- shapes -------------------------------------------------------------------------------------------------------------------------
SHAPES = ("S", "M1", "M2", "G")


def seg_of(threads, k):
    return 2 * k * threads


def n_of(shape, threads, k):
    seg = seg_of(threads, k)
    return {"S": seg - 3, "M1": 2 * seg + 5, "M2": threads * seg + 7, "G": 2 * threads * seg + 7}[shape]


def shape_of(n, seg, threads, no_resident):
    """the launch path of a handle from its geometry (smc_create, step_sys_t in smc_model.hip); R = the LDS-resident kernels"""
    nseg = (n + seg - 1) // seg
    p2 = 1
    while p2 < nseg:
        p2 <<= 1
    if nseg == 1:
        return "S" if no_resident else "R"
    return "M1" if p2 <= threads else "M2" if p2 <= 2 * threads else "G"


def steps_of(n):
    return 4 if n <= (1 << 20) else 3 if n < (1 << 24) else 2


# ---- exclusions ---------------------------------------------------------------------------------------------------------------------
# The oracle costs 0.15 us (LG1D) to 0.25 us (UCSV3D) per particle-step on one core: 1.8 s resp. 3.1 s for 2^22 particles at T = 3.
# Shapes M2 and G grow with threads^2, so at 512 and 1024 threads only these objects keep them; every other shape of every object stays.
KEEP_512 = tuple(("plain", m) for m in FAMILIES["plain"]) + (("guided", 1), ("missing", 1), ("cond", 1))
KEEP_1024 = {"M2": (("plain", 1), ("plain", 3)), "G": (("plain", 1),)}
REASON_COST = "oracle cost: %d particles x %d steps on one CPU core"


def excluded(variant, model, threads, k, shape):
    """the reason a cell is left out, or None"""
    if shape not in ("M2", "G") or threads < 512:
        return None
    keep = KEEP_512 if threads == 512 else KEEP_1024[shape]
    if (variant, model) in keep:
        return None
    n = n_of(shape, threads, k)
    return REASON_COST % (n, steps_of(n))


def unreachable(variant, threads, k, shape):
    """a conditional handle holds at most 2^20 particles: the shapes whose SMALLEST size is beyond that cannot be created"""
    if variant != "cond":
        return False
    seg = seg_of(threads, k)
    least = {"S": 1, "M1": seg + 1, "M2": threads * seg + 1, "G": 2 * threads * seg + 1}[shape]
    return least > COND_MAX_N


EXCLUSIONS = tuple((v, m, th, k, s, excluded(v, m, th, k, s)) for v, m, th, k in STEP_TRIPLES for s in SHAPES
                   if excluded(v, m, th, k, s) and not unreachable(v, th, k, s))
UNREACHABLE = tuple((v, m, th, k, s) for v, m, th, k in STEP_TRIPLES for s in SHAPES if unreachable(v, th, k, s))

# ---- cases --------------------------------------------------------------------------------------------------------------------------
# mode: "mn" multinomial, two filters with distinct rows; "sys" systematic, two filters; "byv" multinomial, ONE filter, its row by
# value in the kernel arguments (STEP_BYV variants; the others read it through the view); "one": one filter, the large shapes
NONE, AFFINE, OPTIMAL = 0, 1, 2
Case = collections.namedtuple("Case", "variant model kind threads np seg shape n nth mode T no_resident")


def kind_of(variant, model, mode):
    """the proposal of a guided case: LG1D takes AFFINE rows in the multinomial modes and OPTIMAL otherwise, UCSV3D has OPTIMAL only"""
    if variant not in ("guided", "missing_guided"):
        return NONE
    return AFFINE if model == LG1D and mode in ("mn", "one") else OPTIMAL


def step_cases():
    """every case of the step kernels.  missing_guided has no step kernel of its own (LAUNCH_OBJECT): its cases - a flagged handle with
    a proposal - launch the guided object's step at an observation and the missing object's at a gap, in S and M1."""
    out = []
    for v, m in OBJECTS:
        if v == "cond" or defines(v, "step") or v == "missing_guided":
            for th, k in GEOMETRIES:
                for shape in SHAPES:
                    if v == "missing_guided" and shape not in ("S", "M1"):
                        continue
                    if unreachable(v, th, k, shape) or (v != "missing_guided" and excluded(v, m, th, k, shape)):
                        continue
                    n = n_of(shape, th, k)
                    modes = ("one",) if shape in ("M2", "G") else ("mn",) + (("sys",) if STEP_SYS[v] else ()) + (("byv",) if STEP_BYV[v] else ())
                    for mode in modes:
                        out.append(Case(v, m, kind_of(v, m, mode), th, k, seg_of(th, k), shape, n, 2 if mode in ("mn", "sys") else 1, mode,
                                        steps_of(n), shape == "S"))
    return out


def cases_per_object():
    """{(variant, model): number of step cases}"""
    c = collections.Counter((x.variant, x.model) for x in step_cases())
    return dict(c)


# ---- the LDS-resident kernels -------------------------------------------------------------------------------------------------------
# Launch<>::resident and ::window (smc_model.hip): (threads, np) by segment length and the answer of resident_np (0 = no preference)
def resident_geo(seg, rnp, window=False):
    if seg == 256:
        return (128, 1)
    if seg == 512:
        return (256, 1)
    if seg == 1024:
        return (512, 1) if rnp == 1 else (128, 4) if rnp == 4 and not window else (256, 2)
    if seg == 2048:
        return (512, 2) if window else (1024, 1) if rnp == 1 else (256, 4) if rnp == 4 else (512, 2)
    if seg == 4096:
        return (512, 4) if rnp == 4 else (1024, 2)
    return (1024, 4)


def resident_np_default(seg, ntheta):
    """resident_np (smc_launch.h) without SMC_RES_NP"""
    return 1 if seg == 1024 and ntheta <= 512 else 0


RESIDENT_SEGS = (1024, 2048, 4096, 8192)


def resident_fits(model, seg):
    """resident_supported (smc_resident.h): 4096 particles for up to three state rows, 8192 for one"""
    return seg <= 2048 or (seg == 4096 and DIM[model] <= 3) or (seg == 8192 and DIM[model] == 1)
