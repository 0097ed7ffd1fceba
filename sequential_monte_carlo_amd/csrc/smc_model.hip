// smc_model.hip -- instantiates the kernels of ONE model family (-DSMC_MODEL=1|2|3|4) for every
// workgroup geometry.  One object per family, built in parallel and linked into libsmchip.so.
#include "smc_launch.h"
#include "smc_forecast_kernels.h"
#include <cstdlib>

#ifndef SMC_MODEL
#error "compile with -DSMC_MODEL=<model id>"
#endif
// -DSMC_GUIDED=1: the same launchers for the GUIDED kernels (handles with a proposal, smc_set_proposal), as translation units
// of their own (build/guided<model>.o): launch_step_g, launch_resident_g, launch_window_g.  Without it: the bootstrap kernels.
#ifndef SMC_GUIDED
#define SMC_GUIDED 0
#endif
#define SMC_G (SMC_GUIDED != 0)
// -DSMC_MISSING=1: the same launchers again for the MISS kernels (handles with SMC_FLAG_NAN_MISSING; smc_spec.h "missing
// observations"), translation units of their own as well: build/missing<model>.o (launch_init_m, launch_step_m, launch_resident_m,
// launch_window_m) and, with -DSMC_GUIDED=1 on top, build/missingg<model>.o (launch_resident_gm, launch_window_gm - the missing
// step itself has no proposal).  Without it: the kernels every other handle launches, untouched by the variant.
#ifndef SMC_MISSING
#define SMC_MISSING 0
#endif
#define SMC_M (SMC_MISSING != 0)
// -DSMC_COND=1: the COND kernels alone (handles with SMC_FLAG_CONDITIONAL; smc_spec.h "the conditional particle filter"):
// build/cond<model>.o with launch_init_c and launch_step_c - one launch per step, multinomial resampling, the filter's stream id
// and rows through the view's pointers.  Nothing else of this file is compiled into those objects.
#ifndef SMC_COND
#define SMC_COND 0
#endif

namespace smc {

#if SMC_COND
template <int THREADS, int NP>
static hipError_t init_c_t(const FilterView& v, int nxt, double y, const double* xrow, hipStream_t s) {
    const size_t lds = scr_words(THREADS, NP) * 8;
    hipLaunchKernelGGL((k_init<SMC_MODEL, THREADS, NP, false, const double*>), dim3(v.nseg, v.ntheta), dim3(THREADS), lds, s, v, nxt, y, xrow);
    return hipGetLastError();
}
template <int THREADS, int NP, bool MULTI, bool GTAB, int RPT>
static hipError_t step_c_launch(const FilterView& v, const StepHot& hot, const double* xrow, int emit_prev, size_t lds, hipStream_t s) {
    static std::atomic<bool> raised[16] = {};   // per instantiation and device
    hipError_t e = raise_lds_limit(k_step_cond<SMC_MODEL, THREADS, NP, MULTI, GTAB, RPT>, lds, raised);
    if (e != hipSuccess) return e;
    const StepLead& l = hot.lead;
    hipLaunchKernelGGL((k_step_cond<SMC_MODEL, THREADS, NP, MULTI, GTAB, RPT>), dim3(v.nseg, v.ntheta), dim3(THREADS), lds, s, l.seed, l.t, l.stream0,
                       l.brow, l.rec0, l.rec1, l.C, step_pack(hot.nseg, hot.cur, emit_prev), l.n32, hot.yval, hot.prm0, v, xrow);
    return hipGetLastError();
}
// (the geometries of step_sys_t below)
template <int THREADS, int NP>
static hipError_t step_c_t(const FilterView& v, const StepHot& hot, const double* xrow, hipStream_t s) {
    if (v.tabD) return step_c_launch<THREADS, NP, true, true, 1>(v, hot, xrow, 0, step_lds_bytes(0, THREADS, NP, true), s);
    const size_t lds = step_lds_bytes(v.nseg_p2, THREADS, NP, v.nseg > 1);
    if (v.nseg_p2 > THREADS) return step_c_launch<THREADS, NP, true, false, 2>(v, hot, xrow, hot.emit_prev, lds, s);
    return v.nseg > 1 ? step_c_launch<THREADS, NP, true, false, 1>(v, hot, xrow, hot.emit_prev, lds, s)
                      : step_c_launch<THREADS, NP, false, false, 1>(v, hot, xrow, hot.emit_prev, lds, s);
}
#define SMC_COND_GEO_SWITCH(FN, ...)                                              \
    switch (g.threads * 8 + g.np) {                                               \
    case 64 * 8 + 2: return FN<64, 2>(__VA_ARGS__);                               \
    case 128 * 8 + 1: return FN<128, 1>(__VA_ARGS__);                             \
    case 128 * 8 + 2: return FN<128, 2>(__VA_ARGS__);                             \
    case 128 * 8 + 4: return FN<128, 4>(__VA_ARGS__);                             \
    case 256 * 8 + 1: return FN<256, 1>(__VA_ARGS__);                             \
    case 256 * 8 + 2: return FN<256, 2>(__VA_ARGS__);                             \
    case 256 * 8 + 4: return FN<256, 4>(__VA_ARGS__);                             \
    case 512 * 8 + 1: return FN<512, 1>(__VA_ARGS__);                             \
    case 512 * 8 + 2: return FN<512, 2>(__VA_ARGS__);                             \
    case 512 * 8 + 4: return FN<512, 4>(__VA_ARGS__);                             \
    case 1024 * 8 + 1: return FN<1024, 1>(__VA_ARGS__);                           \
    case 1024 * 8 + 2: return FN<1024, 2>(__VA_ARGS__);                           \
    case 1024 * 8 + 4: return FN<1024, 4>(__VA_ARGS__);                           \
    }                                                                             \
    return hipErrorInvalidValue;
template <>
hipError_t launch_init_c<SMC_MODEL>(const FilterView& v, Geo g, int nxt, double y, const double* xrow, hipStream_t s) {
    if (!xrow) return hipErrorInvalidValue;
    SMC_COND_GEO_SWITCH(init_c_t, v, nxt, y, xrow, s)
}
template <>
hipError_t launch_step_c<SMC_MODEL>(const FilterView& v, Geo g, const StepHot& hot, const double* xrow, hipStream_t s) {
    if (!xrow || v.systematic) return hipErrorInvalidValue;
    SMC_COND_GEO_SWITCH(step_c_t, v, hot, xrow, s)
}
}  // namespace smc
#else

#if !SMC_G
template <int THREADS, int NP>
static hipError_t init_t(const FilterView& v, int nxt, double y, hipStream_t s) {
    const size_t lds = scr_words(THREADS, NP) * 8;
    hipLaunchKernelGGL((k_init<SMC_MODEL, THREADS, NP, SMC_M>), dim3(v.nseg, v.ntheta), dim3(THREADS), lds, s, v, nxt, y);
    return hipGetLastError();
}
#endif
// one launch of k_step<..., BYV>: the kernel's parameter list is the leading scalars (StepLead) one by one at the head (what the
// wave finds preloaded), the observation, the parameter row, the view
#if SMC_M && !SMC_G
// (the missing step reads the filter's row and stream id through the view on every launch: BYV is not instantiated)
template <int THREADS, int NP, bool MULTI, bool SYS, bool GTAB, int RPT, bool BYV>
static hipError_t step_launch(const FilterView& v, const StepHot& hot, int emit_prev, size_t lds, hipStream_t s) {
    static_assert(!BYV, "missing step: through the pointers");
    static std::atomic<bool> raised[16] = {};   // per instantiation and device
    hipError_t e = raise_lds_limit(k_step_miss<SMC_MODEL, THREADS, NP, MULTI, SYS, GTAB, RPT>, lds, raised);
    if (e != hipSuccess) return e;
    const StepLead& l = hot.lead;
    hipLaunchKernelGGL((k_step_miss<SMC_MODEL, THREADS, NP, MULTI, SYS, GTAB, RPT>), dim3(v.nseg, v.ntheta), dim3(THREADS), lds, s, l.seed, l.t,
                       l.stream0, l.brow, l.rec0, l.rec1, l.C, step_pack(hot.nseg, hot.cur, emit_prev), l.n32, hot.yval, hot.prm0, v);
    return hipGetLastError();
}
#elif !SMC_M
template <int THREADS, int NP, bool MULTI, bool SYS, bool GTAB, int RPT, bool BYV>
static hipError_t step_launch(const FilterView& v, const StepHot& hot, int emit_prev, size_t lds, hipStream_t s) {
    static std::atomic<bool> raised[16] = {};   // per instantiation and device
    hipError_t e = raise_lds_limit(k_step<SMC_MODEL, THREADS, NP, MULTI, SYS, GTAB, RPT, SMC_G, BYV>, lds, raised);
    if (e != hipSuccess) return e;
    const StepLead& l = hot.lead;
    hipLaunchKernelGGL((k_step<SMC_MODEL, THREADS, NP, MULTI, SYS, GTAB, RPT, SMC_G, BYV>), dim3(v.nseg, v.ntheta), dim3(THREADS), lds, s, l.seed, l.t,
                       l.stream0, l.brow, l.rec0, l.rec1, l.C, step_pack(hot.nseg, hot.cur, emit_prev), l.n32, hot.yval, hot.prm0, v);
    return hipGetLastError();
}
#endif
#if !(SMC_M && SMC_G)
template <int THREADS, int NP, bool SYS, bool BYV>
static hipError_t step_sys_t(const FilterView& v, const StepHot& hot, hipStream_t s) {
    if (v.tabD)   // the table comes from k_table (launched by the caller before this step): no table in LDS, nothing to emit
        return step_launch<THREADS, NP, true, SYS, true, 1, BYV>(v, hot, 0, step_lds_bytes(0, THREADS, NP, true), s);
    const size_t lds = step_lds_bytes(v.nseg_p2, THREADS, NP, v.nseg > 1);
    if (v.nseg_p2 > THREADS)   // up to twice as many segments as threads: the window prologue with two records per thread
        return step_launch<THREADS, NP, true, SYS, false, 2, BYV>(v, hot, hot.emit_prev, lds, s);
    return v.nseg > 1 ? step_launch<THREADS, NP, true, SYS, false, 1, BYV>(v, hot, hot.emit_prev, lds, s)
                      : step_launch<THREADS, NP, false, SYS, false, 1, BYV>(v, hot, hot.emit_prev, lds, s);
}
template <int THREADS, int NP>
static hipError_t step_t(const FilterView& v, const StepHot& hot, hipStream_t s) {
#if SMC_M
    return v.systematic ? step_sys_t<THREADS, NP, true, false>(v, hot, s) : step_sys_t<THREADS, NP, false, false>(v, hot, s);
#else
    if (hot.by_value) return v.systematic ? step_sys_t<THREADS, NP, true, true>(v, hot, s) : step_sys_t<THREADS, NP, false, true>(v, hot, s);
    return v.systematic ? step_sys_t<THREADS, NP, true, false>(v, hot, s) : step_sys_t<THREADS, NP, false, false>(v, hot, s);
#endif
}
#endif

#define SMC_GEO_SWITCH(FN, ...)                                                   \
    switch (g.threads * 8 + g.np) {                                               \
    case 64 * 8 + 2: return FN<64, 2>(__VA_ARGS__);                               \
    case 128 * 8 + 1: return FN<128, 1>(__VA_ARGS__);                             \
    case 128 * 8 + 2: return FN<128, 2>(__VA_ARGS__);                             \
    case 128 * 8 + 4: return FN<128, 4>(__VA_ARGS__);                             \
    case 256 * 8 + 1: return FN<256, 1>(__VA_ARGS__);                             \
    case 256 * 8 + 2: return FN<256, 2>(__VA_ARGS__);                             \
    case 256 * 8 + 4: return FN<256, 4>(__VA_ARGS__);                             \
    case 512 * 8 + 1: return FN<512, 1>(__VA_ARGS__);                             \
    case 512 * 8 + 2: return FN<512, 2>(__VA_ARGS__);                             \
    case 512 * 8 + 4: return FN<512, 4>(__VA_ARGS__);                             \
    case 1024 * 8 + 1: return FN<1024, 1>(__VA_ARGS__);                           \
    case 1024 * 8 + 2: return FN<1024, 2>(__VA_ARGS__);                           \
    case 1024 * 8 + 4: return FN<1024, 4>(__VA_ARGS__);                           \
    }                                                                             \
    return hipErrorInvalidValue;

#if !SMC_G && SMC_M
template <>
hipError_t launch_init_m<SMC_MODEL>(const FilterView& v, Geo g, int nxt, double y, hipStream_t s) {
    SMC_GEO_SWITCH(init_t, v, nxt, y, s)
}
#define SMC_LAUNCH_STEP launch_step_m
#define SMC_LAUNCH_RESIDENT launch_resident_m
#define SMC_LAUNCH_WINDOW launch_window_m
#elif !SMC_G
template <>
hipError_t launch_init<SMC_MODEL>(const FilterView& v, Geo g, int nxt, double y, hipStream_t s) {
    SMC_GEO_SWITCH(init_t, v, nxt, y, s)
}
template <int THREADS, int NP>
static hipError_t forecast_t(const FilterView& v, const double* src, uint64_t fseed, uint32_t k0, int nk, double* out, hipStream_t s) {
    hipLaunchKernelGGL((k_forecast<SMC_MODEL, THREADS, NP>), dim3(v.nseg, v.ntheta), dim3(THREADS), 0, s, v, src, fseed, k0, nk, out);
    return hipGetLastError();
}
template <>
hipError_t launch_forecast<SMC_MODEL>(const FilterView& v, Geo g, const double* src, uint64_t fseed, uint32_t k0, int nk, double* out, hipStream_t s) {
    if (2 * g.np * g.threads != v.seg || nk < 1) return hipErrorInvalidValue;   // (a workgroup covers exactly one segment)
    SMC_GEO_SWITCH(forecast_t, v, src, fseed, k0, nk, out, s)
}
#define SMC_LAUNCH_STEP launch_step
#define SMC_LAUNCH_RESIDENT launch_resident
#define SMC_LAUNCH_WINDOW launch_window
#elif SMC_M
#define SMC_LAUNCH_RESIDENT launch_resident_gm
#define SMC_LAUNCH_WINDOW launch_window_gm
#else
#define SMC_LAUNCH_STEP launch_step_g
#define SMC_LAUNCH_RESIDENT launch_resident_g
#define SMC_LAUNCH_WINDOW launch_window_g
#endif
#ifdef SMC_LAUNCH_STEP
template <>
hipError_t SMC_LAUNCH_STEP<SMC_MODEL>(const FilterView& v, Geo g, const StepHot& hot, hipStream_t s) {
    if (hot.by_value && v.ntheta != 1) return hipErrorInvalidValue;   // by value: ONE filter per launch
    SMC_GEO_SWITCH(step_t, v, hot, s)
}
#endif

template <int THREADS, int NP, bool SYS, bool WIN, bool SUMM = false, bool UNW = false>
static hipError_t resident_sys_t(const FilterView& v, int T, StepRec* recs, int t0, int bin, int bout, double* win, hipStream_t s) {
    const size_t lds = resident_lds_bytes<SMC_MODEL>(2 * NP * THREADS, THREADS, NP, SUMM ? v.sum_np : -1);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    static std::atomic<bool> raised[16] = {};   // per instantiation and device
    hipError_t e = raise_lds_limit(k_resident<SMC_MODEL, THREADS, NP, SYS, WIN, SUMM, UNW, SMC_G, SMC_M>, lds, raised);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_resident<SMC_MODEL, THREADS, NP, SYS, WIN, SUMM, UNW, SMC_G, SMC_M>), dim3(v.ntheta), dim3(THREADS), lds, s, v, T, recs, t0, bin, bout, win);
    return hipGetLastError();
}
// per-step summaries (smc_set_summaries) select the SUMM kernels; they exist for the multinomial default only (the C ABI sends
// a systematic filter with summaries through the one-launch-per-step path); the summary mode (sum_unw) selects their UNW twins
template <int THREADS, int NP>
static hipError_t resident_t(const FilterView& v, int T, StepRec* recs, hipStream_t s) {
    if ((v.sum_np || v.sum_mom) && v.sum_unw) return resident_sys_t<THREADS, NP, false, false, true, true>(v, T, recs, 0, 0, 0, nullptr, s);
    if (v.sum_np || v.sum_mom) return resident_sys_t<THREADS, NP, false, false, true>(v, T, recs, 0, 0, 0, nullptr, s);
    return v.systematic ? resident_sys_t<THREADS, NP, true, false>(v, T, recs, 0, 0, 0, nullptr, s)
                        : resident_sys_t<THREADS, NP, false, false>(v, T, recs, 0, 0, 0, nullptr, s);
}
template <int THREADS, int NP>
static hipError_t window_t(const FilterView& v, int T, StepRec* recs, int t0, int bin, int bout, double* win, hipStream_t s) {
    if ((v.sum_np || v.sum_mom) && v.sum_unw) return resident_sys_t<THREADS, NP, false, true, true, true>(v, T, recs, t0, bin, bout, win, s);
    if (v.sum_np || v.sum_mom) return resident_sys_t<THREADS, NP, false, true, true>(v, T, recs, t0, bin, bout, win, s);
    return v.systematic ? resident_sys_t<THREADS, NP, true, true>(v, T, recs, t0, bin, bout, win, s)
                        : resident_sys_t<THREADS, NP, false, true>(v, T, recs, t0, bin, bout, win, s);
}

// threads / particle pairs per thread of the LDS-resident kernels for a segment length.  Measured (scripts/res_tune.py,
// scripts/prof_c2.py, scripts/dbg/res1024.py): with at most two workgroups per CU in flight (n_theta <= 512) every model runs faster
// with one pair per thread (twice the waves: 512 UCSV filters 2.05 -> 1.81 ms); beyond, workgroups of half the size with two
// pairs per thread pack the CUs without a ragged last round (576 .. 768 filters: +30 % LG, +11 % UCSV; 1024: +8 %).  SMC_RES_NP
// (1, 2 or 4) overrides the choice for tuning runs; results do not depend on it (tests/test_gpu_parity.py::test_launch_geometry_knobs).
static int resident_np(const FilterView& v) {
    const char* e = getenv("SMC_RES_NP");
    return e ? atoi(e) : (v.seg == 1024 && v.ntheta <= 512) ? 1 : 0;
}

template <>
hipError_t SMC_LAUNCH_RESIDENT<SMC_MODEL>(const FilterView& v, int T, StepRec* recs, hipStream_t s) {
    const int np = resident_np(v);
    switch (v.seg) {
    case 256: return resident_t<128, 1>(v, T, recs, s);
    case 512: return resident_t<256, 1>(v, T, recs, s);
    case 1024: return np == 1 ? resident_t<512, 1>(v, T, recs, s) : np == 4 ? resident_t<128, 4>(v, T, recs, s) : resident_t<256, 2>(v, T, recs, s);
    case 2048: return np == 1 ? resident_t<1024, 1>(v, T, recs, s) : np == 4 ? resident_t<256, 4>(v, T, recs, s) : resident_t<512, 2>(v, T, recs, s);
    case 4096:   // (four state rows: 4096 particles and their prefix sums exceed the 160 KiB of LDS - resident_supported says so first)
        if constexpr (model_dim<SMC_MODEL>::value > 3) return hipErrorInvalidValue;
        else return np == 4 ? resident_t<512, 4>(v, T, recs, s) : resident_t<1024, 2>(v, T, recs, s);   // (1024 x 2 spills a little and still wins: +5-10 %, scripts/dbg/res4096.py)
    case 8192:
        if constexpr (model_dim<SMC_MODEL>::value == 1) return resident_t<1024, 4>(v, T, recs, s);
        else return hipErrorInvalidValue;
    }
    return hipErrorInvalidValue;
}

#if !SMC_G && !SMC_M
template <int THREADS, int NP, bool UNW>
static hipError_t summ_once_m(const FilterView& v, int cur, hipStream_t s) {
    constexpr int D = model_dim<SMC_MODEL>::value;
    const size_t lds = summ_once_lds_bytes<D>(2 * NP * THREADS, v.sum_np);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    static std::atomic<bool> raised[16] = {};
    hipError_t e = raise_lds_limit(k_summ_once<THREADS, NP, D, UNW>, lds, raised);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_summ_once<THREADS, NP, D, UNW>), dim3(v.ntheta), dim3(THREADS), lds, s, v, cur);
    return hipGetLastError();
}
template <int THREADS, int NP>
static hipError_t summ_once_t(const FilterView& v, int cur, hipStream_t s) {
    return v.sum_unw ? summ_once_m<THREADS, NP, true>(v, cur, s) : summ_once_m<THREADS, NP, false>(v, cur, s);
}
template <>
hipError_t launch_summ_once<SMC_MODEL>(const FilterView& v, int cur, hipStream_t s) {
    if (v.nseg != 1) return hipErrorInvalidValue;
    switch (v.seg) {
    case 256: return summ_once_t<128, 1>(v, cur, s);
    case 512: return summ_once_t<256, 1>(v, cur, s);
    case 1024: return summ_once_t<512, 1>(v, cur, s);
    case 2048: return summ_once_t<512, 2>(v, cur, s);
    case 4096:
        if constexpr (model_dim<SMC_MODEL>::value > 3) return hipErrorInvalidValue;   // (does not fit LDS: the streaming kernels serve it)
        else return summ_once_t<512, 4>(v, cur, s);
    case 8192:
        if constexpr (model_dim<SMC_MODEL>::value > 3) return hipErrorInvalidValue;
        else return summ_once_t<1024, 4>(v, cur, s);
    }
    return hipErrorInvalidValue;
}
#endif

template <>
hipError_t SMC_LAUNCH_WINDOW<SMC_MODEL>(const FilterView& v, int T, StepRec* recs, int t0, int bin, int bout, double* win, hipStream_t s) {
    const int np = resident_np(v);
    switch (v.seg) {
    case 256: return window_t<128, 1>(v, T, recs, t0, bin, bout, win, s);
    case 512: return window_t<256, 1>(v, T, recs, t0, bin, bout, win, s);
    case 1024: return np == 1 ? window_t<512, 1>(v, T, recs, t0, bin, bout, win, s) : window_t<256, 2>(v, T, recs, t0, bin, bout, win, s);
    case 2048: return window_t<512, 2>(v, T, recs, t0, bin, bout, win, s);
    case 4096:
        if constexpr (model_dim<SMC_MODEL>::value > 3) return hipErrorInvalidValue;
        else return np == 4 ? window_t<512, 4>(v, T, recs, t0, bin, bout, win, s) : window_t<1024, 2>(v, T, recs, t0, bin, bout, win, s);
    case 8192:
        if constexpr (model_dim<SMC_MODEL>::value == 1) return window_t<1024, 4>(v, T, recs, t0, bin, bout, win, s);
        else return hipErrorInvalidValue;
    }
    return hipErrorInvalidValue;
}

}  // namespace smc
#endif   // !SMC_COND
