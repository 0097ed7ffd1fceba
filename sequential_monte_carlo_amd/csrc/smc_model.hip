// smc_model.hip -- instantiates the kernels of ONE variant of ONE model family (-DSMC_VARIANT=<Variant id, smc_launch.h>
// -DSMC_MODEL=1|2|3|4) for every workgroup geometry, behind Launch<SMC_MODEL, SMC_VARIANT>.  One object per pair (KERNELS in the
// Makefile, LAUNCH_FAMILIES in smc_launch.h), built in parallel and linked into libsmchip.so.
#include "smc_launch.h"
#include "smc_forecast_kernels.h"
#include <cstdlib>

#ifndef SMC_MODEL
#error "compile with -DSMC_MODEL=<model id>"
#endif
#ifndef SMC_VARIANT   // (the plain kernels: what scripts/dbg/isa.sh and a bare -DSMC_MODEL=<id> compile)
#define SMC_VARIANT 0
#endif

namespace smc {

// What the variant makes of the kernels below; which entry points this object defines: launch_defines (smc_launch.h).
// Everything that depends on these is selected with if constexpr INSIDE templates: a discarded branch instantiates no kernel.
constexpr int VAR = SMC_VARIANT;
constexpr bool VAR_GUIDED = VAR == VARIANT_GUIDED || VAR == VARIANT_MISSING_GUIDED;   // k_step / k_resident<..., GUIDED>
constexpr bool VAR_MISS = VAR == VARIANT_MISSING || VAR == VARIANT_MISSING_GUIDED;    // k_init<..., MISS>, k_step_miss, k_resident<..., MISS>
constexpr bool VAR_COND = VAR == VARIANT_COND;   // k_init<..., const double*> and k_step_cond: the reference row as their last argument
// the missing step reads the filter's row and stream id through the view on every launch, and so does the conditional step,
// which resamples by the multinomial law only: BYV resp. SYS are not instantiated for them
constexpr bool STEP_BYV = !VAR_MISS && !VAR_COND;
constexpr bool STEP_SYS = !VAR_COND;
static_assert(launch_has_object(VAR, SMC_MODEL), "this (variant, family) pair is not in LAUNCH_FAMILIES (smc_launch.h)");

template <int THREADS, int NP>
static hipError_t init_t(const FilterView& v, int nxt, double y, const double* xrow, hipStream_t s) {
    const size_t lds = scr_words(THREADS, NP) * 8;
    if constexpr (VAR_COND) hipLaunchKernelGGL((k_init<SMC_MODEL, THREADS, NP, false, const double*>), dim3(v.nseg, v.ntheta), dim3(THREADS), lds, s, v, nxt, y, xrow);
    else hipLaunchKernelGGL((k_init<SMC_MODEL, THREADS, NP, VAR_MISS>), dim3(v.nseg, v.ntheta), dim3(THREADS), lds, s, v, nxt, y);
    return hipGetLastError();
}
template <int THREADS, int NP, bool MULTI, bool SYS, bool GTAB, int RPT, bool BYV>
constexpr auto step_kernel() {
    if constexpr (VAR_COND) return &k_step_cond<SMC_MODEL, THREADS, NP, MULTI, GTAB, RPT>;
    else if constexpr (VAR_MISS) return &k_step_miss<SMC_MODEL, THREADS, NP, MULTI, SYS, GTAB, RPT>;
    else return &k_step<SMC_MODEL, THREADS, NP, MULTI, SYS, GTAB, RPT, VAR_GUIDED, BYV>;
}
// one launch of the step kernel: its parameter list is the leading scalars (StepLead) one by one at the head (what the wave finds
// preloaded), the observation, the parameter row, the view (and the reference row, conditional)
template <int THREADS, int NP, bool MULTI, bool SYS, bool GTAB, int RPT, bool BYV>
static hipError_t step_launch(const FilterView& v, const StepHot& hot, const double* xrow, int emit_prev, size_t lds, hipStream_t s) {
    static_assert((STEP_SYS || !SYS) && (STEP_BYV || !BYV), "not instantiated for this variant");
    constexpr auto kernel = step_kernel<THREADS, NP, MULTI, SYS, GTAB, RPT, BYV>();
    static std::atomic<bool> raised[16] = {};   // per instantiation and device
    hipError_t e = raise_lds_limit(kernel, lds, raised);
    if (e != hipSuccess) return e;
    const StepLead& l = hot.lead;
    auto launch = [&](auto... tail) {
        hipLaunchKernelGGL(kernel, dim3(v.nseg, v.ntheta), dim3(THREADS), lds, s, l.seed, l.t, l.stream0, l.brow, l.rec0, l.rec1, l.C,
                           step_pack(hot.nseg, hot.cur, emit_prev), l.n32, hot.yval, hot.prm0, v, tail...);
    };
    if constexpr (VAR_COND) launch(xrow);
    else launch();
    return hipGetLastError();
}
template <int THREADS, int NP, bool SYS, bool BYV>
static hipError_t step_sys_t(const FilterView& v, const StepHot& hot, const double* xrow, hipStream_t s) {
    // A conditional handle holds at most PATH_MAX_N particles (smc_create refuses more): a table shape that takes more segments of
    // this length than that many particles fill is never launched for it, and not instantiated (DESIGN.md 2l lists them)
    constexpr int64_t SEG = 2 * NP * THREADS;
    constexpr bool HAS_GTAB = !VAR_COND || 2 * THREADS * SEG < PATH_MAX_N;   // (more than 2 THREADS segments)
    constexpr bool HAS_RPT2 = !VAR_COND || THREADS * SEG < PATH_MAX_N;       // (more than THREADS segments)
    if (v.tabD) {   // the table comes from k_table (launched by the caller before this step): no table in LDS, nothing to emit
        if constexpr (HAS_GTAB) return step_launch<THREADS, NP, true, SYS, true, 1, BYV>(v, hot, xrow, 0, step_lds_bytes(0, THREADS, NP, true), s);
        else return hipErrorInvalidValue;
    }
    const size_t lds = step_lds_bytes(v.nseg_p2, THREADS, NP, v.nseg > 1);
    if (v.nseg_p2 > THREADS) {   // up to twice as many segments as threads: the window prologue with two records per thread
        if constexpr (HAS_RPT2) return step_launch<THREADS, NP, true, SYS, false, 2, BYV>(v, hot, xrow, hot.emit_prev, lds, s);
        else return hipErrorInvalidValue;
    }
    return v.nseg > 1 ? step_launch<THREADS, NP, true, SYS, false, 1, BYV>(v, hot, xrow, hot.emit_prev, lds, s)
                      : step_launch<THREADS, NP, false, SYS, false, 1, BYV>(v, hot, xrow, hot.emit_prev, lds, s);
}
template <int THREADS, int NP>
static hipError_t step_t(const FilterView& v, const StepHot& hot, const double* xrow, hipStream_t s) {
    if constexpr (STEP_BYV)
        if (hot.by_value) return v.systematic ? step_sys_t<THREADS, NP, true, true>(v, hot, xrow, s) : step_sys_t<THREADS, NP, false, true>(v, hot, xrow, s);
    if constexpr (STEP_SYS)
        if (v.systematic) return step_sys_t<THREADS, NP, true, false>(v, hot, xrow, s);
    return step_sys_t<THREADS, NP, false, false>(v, hot, xrow, s);
}
template <int THREADS, int NP>
static hipError_t forecast_t(const FilterView& v, const double* src, uint64_t fseed, uint32_t k0, int nk, double* out, hipStream_t s) {
    hipLaunchKernelGGL((k_forecast<SMC_MODEL, THREADS, NP>), dim3(v.nseg, v.ntheta), dim3(THREADS), 0, s, v, src, fseed, k0, nk, out);
    return hipGetLastError();
}

// The instantiated geometries of the one-launch-per-step kernels (what geo_valid, smc_capi.hip, accepts is this list)
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
    }

// The entry points.  Templates only for the sake of if constexpr: instantiated for <SMC_MODEL, VAR> alone, at the end of this file.
template <int MODEL, int VARIANT>
hipError_t Launch<MODEL, VARIANT>::init(const FilterView& v, Geo g, int nxt, double y, const double* xrow, hipStream_t s) {
    if constexpr (launch_defines(VARIANT, ENTRY_INIT)) {
        if (VAR_COND && !xrow) return hipErrorInvalidValue;
        SMC_GEO_SWITCH(init_t, v, nxt, y, xrow, s)
    }
    return hipErrorInvalidValue;
}
template <int MODEL, int VARIANT>
hipError_t Launch<MODEL, VARIANT>::step(const FilterView& v, Geo g, const StepHot& hot, const double* xrow, hipStream_t s) {
    if constexpr (launch_defines(VARIANT, ENTRY_STEP)) {
        if (VAR_COND && (!xrow || v.systematic)) return hipErrorInvalidValue;
        if (!VAR_COND && hot.by_value && v.ntheta != 1) return hipErrorInvalidValue;   // by value: ONE filter per launch
        SMC_GEO_SWITCH(step_t, v, hot, xrow, s)
    }
    return hipErrorInvalidValue;
}
template <int MODEL, int VARIANT>
hipError_t Launch<MODEL, VARIANT>::forecast(const FilterView& v, Geo g, const double* src, uint64_t fseed, uint32_t k0, int nk, double* out, hipStream_t s) {
    if constexpr (launch_defines(VARIANT, ENTRY_FORECAST)) {
        if (2 * g.np * g.threads != v.seg || nk < 1) return hipErrorInvalidValue;   // (a workgroup covers exactly one segment)
        SMC_GEO_SWITCH(forecast_t, v, src, fseed, k0, nk, out, s)
    }
    return hipErrorInvalidValue;
}

template <int THREADS, int NP, bool SYS, bool WIN, bool SUMM = false, bool UNW = false>
static hipError_t resident_sys_t(const FilterView& v, int T, StepRec* recs, int t0, int bin, int bout, double* win, hipStream_t s) {
    const size_t lds = resident_lds_bytes<SMC_MODEL>(2 * NP * THREADS, THREADS, NP, SUMM ? v.sum_np : -1);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    static std::atomic<bool> raised[16] = {};   // per instantiation and device
    hipError_t e = raise_lds_limit(k_resident<SMC_MODEL, THREADS, NP, SYS, WIN, SUMM, UNW, VAR_GUIDED, VAR_MISS>, lds, raised);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_resident<SMC_MODEL, THREADS, NP, SYS, WIN, SUMM, UNW, VAR_GUIDED, VAR_MISS>), dim3(v.ntheta), dim3(THREADS), lds, s, v, T, recs, t0, bin, bout, win);
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

// threads / particle pairs per thread of the LDS-resident kernels for a segment length: by resident_np (smc_launch.h).
// (the geometry tables of resident and window differ on purpose: window has no np == 4 at 1024 and only 512 x 2 at 2048)
template <int MODEL, int VARIANT>
hipError_t Launch<MODEL, VARIANT>::resident(const FilterView& v, int T, StepRec* recs, hipStream_t s) {
    if constexpr (launch_defines(VARIANT, ENTRY_RESIDENT)) {
        const int np = resident_np(v);
        switch (v.seg) {
        case 256: return resident_t<128, 1>(v, T, recs, s);
        case 512: return resident_t<256, 1>(v, T, recs, s);
        case 1024: return np == 1 ? resident_t<512, 1>(v, T, recs, s) : np == 4 ? resident_t<128, 4>(v, T, recs, s) : resident_t<256, 2>(v, T, recs, s);
        case 2048: return np == 1 ? resident_t<1024, 1>(v, T, recs, s) : np == 4 ? resident_t<256, 4>(v, T, recs, s) : resident_t<512, 2>(v, T, recs, s);
        case 4096:   // (four state rows: 4096 particles and their prefix sums exceed the 160 KiB of LDS - resident_supported says so first)
            if constexpr (model_dim<MODEL>::value > 3) return hipErrorInvalidValue;
            else return np == 4 ? resident_t<512, 4>(v, T, recs, s) : resident_t<1024, 2>(v, T, recs, s);   // (1024 x 2 spills a little and still wins: +5-10 %, scripts/dbg/res4096.py)
        case 8192:
            if constexpr (model_dim<MODEL>::value == 1) return resident_t<1024, 4>(v, T, recs, s);
            else return hipErrorInvalidValue;
        }
    }
    return hipErrorInvalidValue;
}
template <int MODEL, int VARIANT>
hipError_t Launch<MODEL, VARIANT>::window(const FilterView& v, int T, StepRec* recs, int t0, int bin, int bout, double* win, hipStream_t s) {
    if constexpr (launch_defines(VARIANT, ENTRY_WINDOW)) {
        const int np = resident_np(v);
        switch (v.seg) {
        case 256: return window_t<128, 1>(v, T, recs, t0, bin, bout, win, s);
        case 512: return window_t<256, 1>(v, T, recs, t0, bin, bout, win, s);
        case 1024: return np == 1 ? window_t<512, 1>(v, T, recs, t0, bin, bout, win, s) : window_t<256, 2>(v, T, recs, t0, bin, bout, win, s);
        case 2048: return window_t<512, 2>(v, T, recs, t0, bin, bout, win, s);
        case 4096:
            if constexpr (model_dim<MODEL>::value > 3) return hipErrorInvalidValue;
            else return np == 4 ? window_t<512, 4>(v, T, recs, t0, bin, bout, win, s) : window_t<1024, 2>(v, T, recs, t0, bin, bout, win, s);
        case 8192:
            if constexpr (model_dim<MODEL>::value == 1) return window_t<1024, 4>(v, T, recs, t0, bin, bout, win, s);
            else return hipErrorInvalidValue;
        }
    }
    return hipErrorInvalidValue;
}

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
template <int MODEL, int VARIANT>
hipError_t Launch<MODEL, VARIANT>::summ_once(const FilterView& v, int cur, hipStream_t s) {
    if constexpr (launch_defines(VARIANT, ENTRY_SUMM_ONCE)) {
        if (v.nseg != 1) return hipErrorInvalidValue;
        switch (v.seg) {
        case 256: return summ_once_t<128, 1>(v, cur, s);
        case 512: return summ_once_t<256, 1>(v, cur, s);
        case 1024: return summ_once_t<512, 1>(v, cur, s);
        case 2048: return summ_once_t<512, 2>(v, cur, s);
        case 4096:
            if constexpr (model_dim<MODEL>::value > 3) return hipErrorInvalidValue;   // (does not fit LDS: the streaming kernels serve it)
            else return summ_once_t<512, 4>(v, cur, s);
        case 8192:
            if constexpr (model_dim<MODEL>::value > 3) return hipErrorInvalidValue;
            else return summ_once_t<1024, 4>(v, cur, s);
        }
    }
    return hipErrorInvalidValue;
}

// this object's entry points
template struct Launch<SMC_MODEL, VAR>;

}  // namespace smc
