// smc_launch.h -- launch entry points, one explicit specialisation set per model family
// (smc_model.hip is compiled once per model with -DSMC_MODEL=<id>, in parallel).
#pragma once
#include "smc_kernels.h"
#include "smc_resident.h"
#include <atomic>
#include <type_traits>

namespace smc {

// The ONE place that knows the list of model families: turns the runtime id into a compile-time tag and calls f with it,
//     by_model(id, [&](auto M) { return launch_step<decltype(M)::value>(...); })
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

template <int MODEL> hipError_t launch_init(const FilterView& v, Geo g, int nxt, double y, hipStream_t s);
// hot: the launch's by-value arguments (StepHot, smc_kernels.h); hot.lead repeats the view's seed and carries the addresses of the
// kernel's early loads as the caller derived them for THIS launch (the view's pointers, the current buffer, t)
template <int MODEL> hipError_t launch_step(const FilterView& v, Geo g, const StepHot& hot, hipStream_t s);
template <int MODEL> hipError_t launch_resident(const FilterView& v, int T, StepRec* recs, hipStream_t s);
// summaries (quantile levels / moments named by the view's sum_* fields, row 0) of the current state of single-segment filters in
// one launch; hipErrorInvalidValue when the segment length has no instantiation or the state does not fit LDS
template <int MODEL> hipError_t launch_summ_once(const FilterView& v, int cur, hipStream_t s);
// window mode: steps [t0, t0 + T) from the state in buffer bin to buffer bout, (logmu, ess) of every step to win
template <int MODEL> hipError_t launch_window(const FilterView& v, int T, StepRec* recs, int t0, int bin, int bout, double* win, hipStream_t s);
// the same three for a handle with a proposal (smc_set_proposal): the GUIDED kernels, instantiated for the families that have
// proposals (LG1D, UCSV3D) in translation units of their own (smc_model.hip with -DSMC_GUIDED=1)
template <int MODEL> hipError_t launch_step_g(const FilterView& v, Geo g, const StepHot& hot, hipStream_t s);
template <int MODEL> hipError_t launch_resident_g(const FilterView& v, int T, StepRec* recs, hipStream_t s);
// forecasts (smc_forecast_kernels.h): nk horizons k0 .. k0 + nk - 1 of every particle from the state rows src [d][ntheta][npad] into
// out [nk][d + 3][ntheta][npad]; hipErrorInvalidValue when g is not the geometry of the view's segment length
template <int MODEL> hipError_t launch_forecast(const FilterView& v, Geo g, const double* src, uint64_t fseed, uint32_t k0, int nk, double* out, hipStream_t s);
template <int MODEL> hipError_t launch_window_g(const FilterView& v, int T, StepRec* recs, int t0, int bin, int bout, double* win, hipStream_t s);
// missing observations (smc_spec.h; handles with SMC_FLAG_NAN_MISSING): the MISS kernels, translation units of their own
// (smc_model.hip with -DSMC_MISSING=1).  launch_init_m / launch_step_m: the missing step itself, launched for a step whose
// observation is NaN (a guided handle too: a missing step has no proposal).  launch_resident_m / launch_window_m: the LDS-resident
// loop that tests every step's observation, launched when the series or window holds a NaN; _gm: their twins for a handle with
// a proposal (bootstrap step at gaps, guided step elsewhere; the families of by_guided_model)
template <int MODEL> hipError_t launch_init_m(const FilterView& v, Geo g, int nxt, double y, hipStream_t s);
template <int MODEL> hipError_t launch_step_m(const FilterView& v, Geo g, const StepHot& hot, hipStream_t s);
template <int MODEL> hipError_t launch_resident_m(const FilterView& v, int T, StepRec* recs, hipStream_t s);
template <int MODEL> hipError_t launch_window_m(const FilterView& v, int T, StepRec* recs, int t0, int bin, int bout, double* win, hipStream_t s);
template <int MODEL> hipError_t launch_resident_gm(const FilterView& v, int T, StepRec* recs, hipStream_t s);
template <int MODEL> hipError_t launch_window_gm(const FilterView& v, int T, StepRec* recs, int t0, int bin, int bout, double* win, hipStream_t s);
// the conditional particle filter (smc_spec.h; handles with SMC_FLAG_CONDITIONAL): the COND kernels, translation units of their
// own (smc_model.hip with -DSMC_COND=1: build/cond<model>.o), for the families of by_density_model.  One launch per step only;
// xrow [d][ntheta]: the reference row of the step on the device (xref + t d ntheta)
template <int MODEL> hipError_t launch_init_c(const FilterView& v, Geo g, int nxt, double y, const double* xrow, hipStream_t s);
template <int MODEL> hipError_t launch_step_c(const FilterView& v, Geo g, const StepHot& hot, const double* xrow, hipStream_t s);

}  // namespace smc
