// smc_launch.h -- the launch entry points of the kernel objects: Launch<MODEL, VARIANT>, one explicit instantiation per
// (variant, model family) pair of LAUNCH_FAMILIES (smc_model.hip is compiled once per pair with -DSMC_VARIANT=<id>
// -DSMC_MODEL=<id>, in parallel), and by_variant, which turns the two run-time ids into that type.
#pragma once
#include "smc_kernels.h"
#include "smc_resident.h"
#include <atomic>
#include <cstdlib>
#include <type_traits>

namespace smc {

// The ONE place that knows the list of model families: turns the runtime id into a compile-time tag and calls f with it,
//     by_model(id, [&](auto M) { return path_step<decltype(M)::value>(...); })
// hipErrorInvalidValue for an id that names no family.  A new family is one line here (and its object in the Makefile).
template <class F>
inline hipError_t by_model(int id, F&& f) {
    switch (id) {
    case MODEL_LG1D: return f(std::integral_constant<int, MODEL_LG1D>{});
    case MODEL_SV1D: return f(std::integral_constant<int, MODEL_SV1D>{});
    case MODEL_UCSV3D: return f(std::integral_constant<int, MODEL_UCSV3D>{});
    case MODEL_UCSV_RB: return f(std::integral_constant<int, MODEL_UCSV_RB>{});
    }
    return hipErrorInvalidValue;
}
// ... and the families that have proposals (proposal_supported, smc_spec.h): the GUIDED kernels exist for these
template <class F>
inline hipError_t by_guided_model(int id, F&& f) {
    switch (id) {
    case MODEL_LG1D: return f(std::integral_constant<int, MODEL_LG1D>{});
    case MODEL_UCSV3D: return f(std::integral_constant<int, MODEL_UCSV3D>{});
    }
    return hipErrorInvalidValue;
}
// ... and the families whose state rows have a transition density (smooth_row, smc_spec.h, yields their constants): the smoother
// and backward simulation, on the device and in their host twins, exist for these
template <class F>
inline hipError_t by_density_model(int id, F&& f) {
    switch (id) {
    case MODEL_LG1D: return f(std::integral_constant<int, MODEL_LG1D>{});
    case MODEL_SV1D: return f(std::integral_constant<int, MODEL_SV1D>{});
    case MODEL_UCSV3D: return f(std::integral_constant<int, MODEL_UCSV3D>{});
    }
    return hipErrorInvalidValue;
}
inline bool has_density(int id) {
    return by_density_model(id, [](auto) { return hipSuccess; }) == hipSuccess;
}

// Kernels that ask for more than the default 64 KiB of dynamic LDS.  The attribute is per device: raise it wherever this
// process has not done so yet (cheap: a table lookup afterwards).  raised: one table per kernel instantiation, atomic because
// handles of different host threads launch the same instantiation (DESIGN.md "Host threads"); two threads that both find it
// unset both raise the limit, which is harmless.
template <class K>
inline hipError_t raise_lds_limit(K kernel, size_t lds, std::atomic<bool> (&raised)[16]) {
    if (lds <= 64 * 1024) return hipSuccess;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < 16 && raised[dev].load(std::memory_order_acquire)) return hipSuccess;
    e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e == hipSuccess && dev >= 0 && dev < 16) raised[dev].store(true, std::memory_order_release);
    return e;
}

// geometry of a workgroup: SEG = 2 * np * threads
struct Geo {
    int threads, np;
};
// the default geometry of a segment size, and whether (threads, np) is an instantiated one
bool geo_default(int seg, Geo& g);
bool geo_valid(int seg, int np, Geo& g);
// Particle pairs per thread of the LDS-resident kernels (Launch<>::resident / ::window pick (threads, np) for the view's segment
// length by it; 0: no preference, the table's own choice).  Measured (scripts/res_tune.py, scripts/prof_c2.py,
// scripts/dbg/res1024.py): with at most two workgroups per CU in flight (n_theta <= 512) every model runs faster with one pair per
// thread (twice the waves: 512 UCSV filters 2.05 -> 1.81 ms); beyond, workgroups of half the size with two pairs per thread pack
// the CUs without a ragged last round (576 .. 768 filters: +30 % LG, +11 % UCSV; 1024: +8 %).  SMC_RES_NP (1, 2 or 4), read at
// every launch, overrides the choice for tuning runs; results do not depend on it (tests/test_gpu_geometry.py).  The ONE statement
// of the rule: the launchers and smc_get_launch_geometry call it.
inline int resident_np(const FilterView& v) {
    const char* e = getenv("SMC_RES_NP");
    return e ? atoi(e) : (v.seg == 1024 && v.ntheta <= 512) ? 1 : 0;
}

// ---- kernel variants ---------------------------------------------------------------------------------
// What a handle's options make of its kernels; every variant is a set of translation units of its own (never a run-time branch
// in the bodies the other handles run).  The ids are the Makefile's -DSMC_VARIANT.
enum Variant : int {
    VARIANT_PLAIN = 0,            // the bootstrap kernels
    VARIANT_GUIDED = 1,           // handles with a proposal (smc_set_proposal): the GUIDED kernels
    VARIANT_MISSING = 2,          // SMC_FLAG_NAN_MISSING (smc_spec.h "missing observations"): the missing step, launched for a step
                                  // whose observation is NaN, and the LDS-resident loops that test every step's observation
    VARIANT_MISSING_GUIDED = 3,   // ... those loops for a handle with a proposal (bootstrap step at gaps, guided step elsewhere)
    VARIANT_COND = 4,             // SMC_FLAG_CONDITIONAL (smc_spec.h "the conditional particle filter"): one launch per step only
    VARIANT_COUNT
};
enum Entry : int { ENTRY_INIT, ENTRY_STEP, ENTRY_RESIDENT, ENTRY_WINDOW, ENTRY_FORECAST, ENTRY_SUMM_ONCE, ENTRY_COUNT };
constexpr int NO_OBJECT = -1;
// The (variant, family) pairs that have an object, one bit per model id - the SAME list as KERNELS in the Makefile: a pair
// missing there is an undefined symbol when the library is loaded, a pair missing here a static_assert in smc_model.hip.
// Guided: the families with proposals (by_guided_model); conditional: those with a transition density (by_density_model).
constexpr unsigned family_bits(int a, int b = 0, int c = 0, int d = 0) { return (1u << a | 1u << b | 1u << c | 1u << d) & ~1u; }
constexpr unsigned LAUNCH_FAMILIES[VARIANT_COUNT] = {
    /* plain          */ family_bits(MODEL_LG1D, MODEL_SV1D, MODEL_UCSV3D, MODEL_UCSV_RB),
    /* guided         */ family_bits(MODEL_LG1D, MODEL_UCSV3D),
    /* missing        */ family_bits(MODEL_LG1D, MODEL_SV1D, MODEL_UCSV3D, MODEL_UCSV_RB),
    /* missing+guided */ family_bits(MODEL_LG1D, MODEL_UCSV3D),
    /* conditional    */ family_bits(MODEL_LG1D, MODEL_SV1D, MODEL_UCSV3D),
};
// ... and the variant whose object serves each entry point of a variant: itself where its object defines the entry point, another
// where the kernels would be the same ones (a first step has no proposal; neither has a missing step), none where the handle
// has no such launch (a conditional handle; forecasts and one-launch summaries run the plain kernels whatever the handle)
// (missing init: the first step of a flagged handle whose first observation is NaN - the gap bit of pick_variant, smc_host.h)
constexpr int LAUNCH_OBJECT[VARIANT_COUNT][ENTRY_COUNT] = {
    //                     init             step             resident                window                  forecast       summ_once
    /* plain          */ {VARIANT_PLAIN,   VARIANT_PLAIN,   VARIANT_PLAIN,          VARIANT_PLAIN,          VARIANT_PLAIN, VARIANT_PLAIN},
    /* guided         */ {VARIANT_PLAIN,   VARIANT_GUIDED,  VARIANT_GUIDED,         VARIANT_GUIDED,         NO_OBJECT,     NO_OBJECT},
    /* missing        */ {VARIANT_MISSING, VARIANT_MISSING, VARIANT_MISSING,        VARIANT_MISSING,        NO_OBJECT,     NO_OBJECT},
    /* missing+guided */ {VARIANT_MISSING, VARIANT_MISSING, VARIANT_MISSING_GUIDED, VARIANT_MISSING_GUIDED, NO_OBJECT,     NO_OBJECT},
    /* conditional    */ {VARIANT_COND,    VARIANT_COND,    NO_OBJECT,              NO_OBJECT,              NO_OBJECT,     NO_OBJECT},
};
constexpr bool launch_has_object(int variant, int model) { return model > 0 && model < 32 && (LAUNCH_FAMILIES[variant] >> model & 1u) != 0; }
constexpr bool launch_defines(int variant, int entry) { return LAUNCH_OBJECT[variant][entry] == variant; }

// The entry points of the object of one pair (smc_model.hip).  An entry point that launch_defines denies the variant refuses and
// instantiates no kernel; by_variant never names it.
template <int MODEL, int VARIANT>
struct Launch {
    // xrow [d][ntheta]: the reference row of the step on the device (xref + t d ntheta) - the conditional variant's; the others ignore it
    static hipError_t init(const FilterView& v, Geo g, int nxt, double y, const double* xrow, hipStream_t s);
    // hot: the launch's by-value arguments (StepHot, smc_kernels.h); hot.lead repeats the view's seed and carries the addresses of
    // the kernel's early loads as the caller derived them for THIS launch (the view's pointers, the current buffer, t)
    static hipError_t step(const FilterView& v, Geo g, const StepHot& hot, const double* xrow, hipStream_t s);
    static hipError_t resident(const FilterView& v, int T, StepRec* recs, hipStream_t s);
    // window mode: steps [t0, t0 + T) from the state in buffer bin to buffer bout, (logmu, ess) of every step to win
    static hipError_t window(const FilterView& v, int T, StepRec* recs, int t0, int bin, int bout, double* win, hipStream_t s);
    // forecasts (smc_forecast_kernels.h): nk horizons k0 .. k0 + nk - 1 of every particle from the state rows src [d][ntheta][npad]
    // into out [nk][d + 3][ntheta][npad]; hipErrorInvalidValue when g is not the geometry of the view's segment length
    static hipError_t forecast(const FilterView& v, Geo g, const double* src, uint64_t fseed, uint32_t k0, int nk, double* out, hipStream_t s);
    // summaries (quantile levels / moments named by the view's sum_* fields, row 0) of the current state of single-segment filters
    // in one launch; hipErrorInvalidValue when the segment length has no instantiation or the state does not fit LDS
    static hipError_t summ_once(const FilterView& v, int cur, hipStream_t s);
};

// Calls f with the Launch<MODEL, VARIANT> of the object that defines ENTRY for (model id, variant):
//     by_variant<ENTRY_STEP>(id, variant, [&](auto L) { return L.step(...); })
// variant: as LAUNCH_OBJECT gives it (pick_variant, smc_host.h).  hipErrorInvalidValue for a pair without an object.
template <int ENTRY, int VARIANT, class F>
inline hipError_t by_variant_model(int id, F&& f) {
    return by_model(id, [&](auto M) {
        if constexpr (launch_defines(VARIANT, ENTRY) && launch_has_object(VARIANT, decltype(M)::value)) return f(Launch<decltype(M)::value, VARIANT>{});
        else return hipErrorInvalidValue;
    });
}
template <int ENTRY, class F>
inline hipError_t by_variant(int id, int variant, F&& f) {
    switch (variant) {
    case VARIANT_PLAIN: return by_variant_model<ENTRY, VARIANT_PLAIN>(id, f);
    case VARIANT_GUIDED: return by_variant_model<ENTRY, VARIANT_GUIDED>(id, f);
    case VARIANT_MISSING: return by_variant_model<ENTRY, VARIANT_MISSING>(id, f);
    case VARIANT_MISSING_GUIDED: return by_variant_model<ENTRY, VARIANT_MISSING_GUIDED>(id, f);
    case VARIANT_COND: return by_variant_model<ENTRY, VARIANT_COND>(id, f);
    }
    return hipErrorInvalidValue;
}

}  // namespace smc
