// smc_capi.hip -- C ABI (include/smc_hip.h) over the gfx950 kernels in smc_kernels.h: the core of the filter handle.
// Handle-owned device state, one HIP stream per handle, HIP-event timing of every call.
// There is NO CPU fallback: every filter entry point launches HIP kernels or fails.
// (the other entry points on a handle: smc_capi_series.hip, smc_capi_summ.hip, smc_capi_pmmh.hip, smc_capi_slots.hip; smc_host.h)
#include "smc_host.h"
#include "smc_aux_kernels.h"

#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>
#ifdef SMC_ABLATE
#include <algorithm>
#include <cstdio>
#include <map>
#endif

using namespace smc;

static thread_local std::string g_err;
#ifdef SMC_ABLATE
static int h_abl_tmp = 0;
static void abl_report(smc_filter_s* h);   // (at the end of this file)
#endif
int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

// ---- geometry ------------------------------------------------------------------------------
namespace smc {
// (threads, np) is an instantiated geometry: the cases of SMC_GEO_SWITCH (smc_model.hip), which is the other statement of the list
bool geo_valid(int seg, int np, Geo& g) {
    if (np != 1 && np != 2 && np != 4) return false;
    const int th = seg / (2 * np);
    if (th * 2 * np != seg) return false;
    if (!(th == 128 || th == 256 || th == 512 || th == 1024 || (th == 64 && np == 2))) return false;
    g = {th, np};
    return true;
}
bool geo_default(int seg, Geo& g) {
    switch (seg) {
    case 256: g = {128, 1}; return true;
    case 512: g = {256, 1}; return true;
    case 1024: g = {512, 1}; return true;
    case 2048: g = {512, 2}; return true;
    case 4096: g = {1024, 2}; return true;   // (measured: 2^26 particles 1109 -> 1055 us per step against 512 x 4)
    case 8192: g = {1024, 4}; return true;
    }
    return false;
}
}  // namespace smc

// most segments a filter may have (the break points of a step sit in the LDS of k_breaks: 8 B per segment)
constexpr int MAX_NSEG = 16384;
extern "C" int smc_auto_seg(int model_id, int64_t n) {
    // measured (scripts/nx_sweep.py, scripts/dbg/mid_sizes.py, scripts/dbg/ucsv_seg_sweep.py): one segment for as long as the LDS-
    // resident kernels hold the filter (8192 particles of one state coordinate, 4096 of three: the batched callers' shape);
    // above, the SHORTEST segment whose workgroup still has a thread per segment (nseg <= seg / 2 resp. 512: the one-record-per-
    // thread window prologue) - a filter of 2^14..2^18 particles is a handful of workgroups on a 256-CU chip and bound by the
    // life of ONE of them, which shorter segments (fewer particles per workgroup) cut from 9.4 to 6.0-7.3 us per step; then the
    // fastest geometry for as long as the segment count allows - one state coordinate: 2048 (512 threads x two pairs, 12.5 us per
    // 2^20 particles) from 2^19 particles on; three coordinates: 1024 (512 threads x ONE pair: with two pairs the step kernel
    // needs 183 vector registers and a CU holds one workgroup instead of two - 2^20 UCSV particles 2.9 -> 3.4e10 p-steps/s);
    // beyond 512 segments the table of the segments is built once per step by k_table instead of by every workgroup; longer
    // segments keep the count at MAX_NSEG for still larger filters.  The segment length is part of the numerical spec (the CPU
    // restatement used by the tests follows the same rule).
    // (four state rows - the marginal UCSV family - follow the three-row rule with the resident limit their LDS allows: 2048)
    const int dm = model_dim_rt(model_id);
    const bool d3 = dm >= 3;
    if (n > (int64_t)MAX_NSEG * 4096) return 8192;
    if (n > (int64_t)MAX_NSEG * 2048) return 4096;
    if (n > (int64_t)MAX_NSEG * 1024) return 2048;
    if (n > ((int64_t)1 << 19)) return d3 ? 1024 : 2048;
    if (n > ((int64_t)1 << 17)) return 1024;
    if (n > ((int64_t)1 << 15)) return 512;
    if (n > (dm > 3 ? 2048 : d3 ? 4096 : MAX_SEG)) return 256;
    int s = 256;
    while (s < n) s <<= 1;
    return s;
}
extern "C" int smc_model_dim(int id) { return model_dim_rt(id); }
extern "C" int smc_model_nraw(int id) { return model_nraw_rt(id); }
extern "C" const char* smc_last_error(void) { return g_err.c_str(); }
extern "C" const char* smc_version(void) { return "smchip 0.1 (gfx950)"; }
extern "C" int smc_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int cond_refuse(const char* who) {
    return fail(SMC_ESTATE, std::string(who) + ": the handle is conditional (SMC_FLAG_CONDITIONAL): it runs smc_init / smc_step only, one launch per step "
                                               "with the reference pinned, and its logZ is not a likelihood estimate");
}

// ---- kernel dispatch -------------------------------------------------------------------------
// (which kernels a launch means: pick_variant, smc_host.h; a conditional handle's take the reference row of the step as their
// last argument)
hipError_t do_init(smc_filter_s* h, double y) {
    return by_variant<ENTRY_INIT>(h->model, pick_variant(h, ENTRY_INIT, nan_missing(h) && y != y),
                                  [&](auto L) { return L.init(h->v, h->geo, h->cur, y, h->cond.d_xref.as<double>(), h->stream); });
}
// filters with more segments than threads per workgroup (v.tabD): the segment table of the current weights, built once (k_table;
// emit as k_step's emit_prev: 0 nothing, 1 (logmu, ess) from the full records, 2 from the totals)
static hipError_t do_table(smc_filter_s* h, int emit, int first_emit, uint32_t t_emit) {
    constexpr int TH = 1024;
    hipLaunchKernelGGL((k_table<TH>), dim3(h->v.ntheta), dim3(TH), 0, h->stream, h->v, h->cur, emit, first_emit, t_emit);
    return hipGetLastError();
}
// The by-value arguments of the launch of step t (StepHot, smc_kernels.h), derived HERE at every launch from the view, the current
// buffer and t - never kept in the handle: the break points are allocated lazily and refilled (ensure_breaks), the buffers flip, and
// smc_permute, slot copies and the bundle a new handle takes over change what the view's pointers mean.
static StepHot step_hot(const smc_filter_s* h, uint32_t t, int emit_prev, double y, const double* y_host) {
    const FilterView& v = h->v;
    StepHot hot{};
    StepLead& l = hot.lead;
    l.seed = v.seed; l.t = t;
    // the addresses of what the kernel loads before its first draw (StepEarly); filter th adds th (nseg + 1) resp. th nseg, th npad
    const bool breaks = v.nseg > 1 && !v.systematic;   // (as ensure_breaks: the caller has made step t's row current)
    l.brow = breaks ? v.brk + (size_t)(t - v.brk_t0) * (size_t)v.ntheta * ((size_t)v.nseg + 1) : nullptr;
    l.rec0 = v.tabD ? (const void*)v.tabD : (const void*)v.segk[h->cur];
    l.rec1 = v.tabD ? (const void*)v.tabsh : (const void*)v.segS[h->cur];
    l.C = v.C[h->cur];
    l.n32 = (uint32_t)v.n;
    hot.nseg = v.nseg; hot.cur = h->cur; hot.emit_prev = emit_prev; hot.yval = y;
    l.pack = step_pack(hot.nseg, hot.cur, hot.emit_prev);
    // By value: ONE filter, no skip mask in force, the host copies of its row and stream id valid, and the observation
    // at hand (the step API's y, or the host's copy of the series).  The results do not depend on the choice.
    if (hot_legal(h) && !v.skip && (!v.y || y_host)) {
        hot.by_value = 1;
        l.stream0 = h->hot.stream0;
        hot.prm0 = h->hot.prm0;
        if (v.y) hot.yval = y_host[t];
    }
    return hot;
}
hipError_t do_step(smc_filter_s* h, uint32_t t, int emit_prev, double y, const double* y_host) {
    if (h->v.tabD) {
        hipError_t e = do_table(h, emit_prev, t == 1u ? 1 : 0, t - 1u);
        if (e != hipSuccess) return e;
        emit_prev = 0;
    }
    const StepHot hot = step_hot(h, t, emit_prev, y, y_host);
    const double* xrow = nullptr;
    if (conditional(h)) {
        if (!h->cond.d_xref || (int64_t)t >= h->cond.T) return hipErrorInvalidValue;   // (smc_step has refused with a message)
        xrow = h->cond.d_xref.as<double>() + (size_t)t * (size_t)h->d * (size_t)h->v.ntheta;
    }
    // the step API's observation, or the series' (gap_y: set only when a flagged handle's series holds a NaN)
    const bool gap = h->v.y ? (h->gap_y && h->gap_y[t] != h->gap_y[t]) : (nan_missing(h) && y != y);
    return by_variant<ENTRY_STEP>(h->model, pick_variant(h, ENTRY_STEP, gap), [&](auto L) { return L.step(h->v, h->geo, hot, xrow, h->stream); });
}
// Break points of the multinomial resampling steps (multi-segment filters; smc_spec.h): computed by k_breaks
// for a window of steps ahead of time - they depend on (seed, stream, t) only.  Called before every step
// launch; almost always a no-op.
hipError_t ensure_breaks(smc_filter_s* h, uint32_t t, uint32_t t_end) {
    FilterView& v = h->v;
    if (v.nseg <= 1 || v.systematic) return hipSuccess;
    if (h->brk_count && t >= v.brk_t0 && t < v.brk_t0 + h->brk_count) return hipSuccess;
    const size_t per_step = (size_t)v.ntheta * ((size_t)v.nseg + 1);
    if (!h->d_brk) {
        size_t steps = ((size_t)32 << 20) / (per_step * 8);    // <= 32 MiB of break points at a time
        steps = steps < 1 ? 1 : (steps > 1024 ? 1024 : steps);
        hipError_t e = h->d_brk.grow(steps * per_step * 8);
        if (e != hipSuccess) return e;
        h->brk_cap = (uint32_t)steps;
        v.brk = h->d_brk.as<uint64_t>();
    }
    uint32_t cnt = t_end > t ? t_end - t : 1;                  // no further than the caller will go
    cnt = cnt > h->brk_cap ? h->brk_cap : cnt;
    constexpr int TH = 256;
    const size_t lds = ((size_t)v.nseg + 1 + TH / WAVE) * 8;
    static std::atomic<bool> raised[16] = {};   // filters of more than 8187 segments: beyond the default limit of dynamic LDS
    hipError_t e = raise_lds_limit(k_breaks<TH>, lds, raised);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_breaks<TH>), dim3(cnt, v.ntheta), dim3(TH), lds, h->stream, v, t, h->d_brk.as<uint64_t>());
    v.brk_t0 = t;
    h->brk_count = cnt;
    return hipGetLastError();
}
static hipError_t do_window(smc_filter_s* h, int k, int bout) {   // (win.gap: a flagged handle's window with a NaN in it)
    return by_variant<ENTRY_WINDOW>(h->model, pick_variant(h, ENTRY_WINDOW, h->win.gap),
                                    [&](auto L) { return L.window(h->v, k, h->d_recs.as<StepRec>(), (int)h->t, h->cur, bout, h->win.h_out.as<double>(), h->stream); });
}

hipError_t do_finalize(smc_filter_s* h, int first_emit, uint32_t t_emit) {
    if (h->v.tabD) return do_table(h, 1, first_emit, t_emit);   // (no room in LDS for a table of that many segments)
    constexpr int TH = 256;
    const size_t lds = table_lds_bytes(h->v.nseg_p2, TH, 1);
    hipLaunchKernelGGL((k_finalize<TH>), dim3(h->v.ntheta), dim3(TH), lds, h->stream, h->v, h->cur, first_emit, t_emit);
    return hipGetLastError();
}

// ---- lifetime ----------------------------------------------------------------------------------
// What every handle needs and the runtime is slow to give back (hipFree, hipStreamDestroy and hipHostFree made smc_destroy cost
// 0.48 ms - twice the hundred steps of a 1024-particle filter): the slab, the stream, the two events and the pinned mirror of a
// destroyed handle are kept (a few, bounded in bytes) and handed to the next smc_create that fits them.  The blocks MOVE between
// handle, bundle and cache; a bundle that is dropped frees them.  The stream and the events are plain handles here: whoever
// holds the bundle last (smc_destroy, when the cache refuses it) destroys them.
namespace {
struct Bundle {
    int device = -1;
    DevBlock slab;
    PinBlock pin;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    DevBlock d_y, d_recs;   // the series buffer and the per-step records of the whole-series calls (whatever the destroyed handle had grown them to)
    PinBlock h_params;      // pinned twin of the parameter rows
};
struct BundleCache {
    std::mutex mu;
    std::vector<Bundle> free_list;
    size_t bytes = 0;
    static constexpr size_t MAX_BYTES = (size_t)512 << 20, MAX_COUNT = 8;
    bool take(int device, size_t slab_bytes, size_t pin_bytes, Bundle& out) {
        std::lock_guard<std::mutex> g(mu);
        for (size_t i = 0; i < free_list.size(); ++i) {
            Bundle& b = free_list[i];
            if (b.device == device && b.slab.bytes() >= slab_bytes && b.slab.bytes() <= 2 * slab_bytes + 4096 && b.pin.bytes() >= pin_bytes) {
                bytes -= b.slab.bytes();
                out = std::move(b);
                free_list.erase(free_list.begin() + (long)i);
                return true;
            }
        }
        return false;
    }
    bool give(Bundle& b) {   // false: refused, b is untouched
        std::lock_guard<std::mutex> g(mu);
        if (free_list.size() >= MAX_COUNT || bytes + b.slab.bytes() > MAX_BYTES) return false;
        bytes += b.slab.bytes();
        free_list.push_back(std::move(b));
        return true;
    }
};
BundleCache& bundle_cache() { static BundleCache* c = new BundleCache(); return *c; }   // (never destroyed: no runtime calls at exit)
}  // namespace

extern "C" int smc_create(int model_id, int64_t n_theta, int64_t n_x, int seg, uint64_t seed, int device, uint32_t flags,
                          smc_handle* out) {
    if (!out) return fail(SMC_EINVAL, "smc_create: out is NULL");
    *out = nullptr;
    const int d = model_dim_rt(model_id);
    if (d < 0) return fail(SMC_EINVAL, "smc_create: unknown model_id " + std::to_string(model_id));
    if (n_theta <= 0 || n_x <= 0) return fail(SMC_EINVAL, "smc_create: n_theta and n_x must be positive");
    if (n_theta > 65535) return fail(SMC_EINVAL, "smc_create: n_theta > 65535 (grid.y limit); shard theta");
    if (seg == 0) seg = smc_auto_seg(model_id, n_x);
    Geo g;
    if (!geo_default(seg, g)) return fail(SMC_EINVAL, "smc_create: seg must be a power of two in [256,8192]");
#ifdef SMC_ABLATE
    if (const char* e = getenv("SMC_ABL")) h_abl_tmp = atoi(e);
#endif
    if (const char* e = getenv("SMC_NP")) {   // tuning knob: particle pairs per thread (1, 2 or 4)
        Geo g2;
        if (geo_valid(seg, atoi(e), g2)) g = g2;
    }
    const int64_t nseg = (n_x + seg - 1) / seg;
    if (nseg > MAX_NSEG) return fail(SMC_EINVAL, "smc_create: more than 16384 segments; use a larger seg");
    if (n_x > ((int64_t)1 << 31)) return fail(SMC_EINVAL, "smc_create: n_x > 2^31");
    if (flags & SMC_FLAG_ANCESTOR_SAMPLING) {   // ancestor sampling (include/smc_hip.h): a mode of the conditional filter, over recorded ancestors
        if (!(flags & SMC_FLAG_CONDITIONAL))
            return fail(SMC_EINVAL, "smc_create: SMC_FLAG_ANCESTOR_SAMPLING without SMC_FLAG_CONDITIONAL (it redraws the ancestors of a reference trajectory)");
        flags |= SMC_FLAG_ANCESTORS;
    }
    if (flags & SMC_FLAG_CONDITIONAL) {   // the conditional particle filter (include/smc_hip.h): what it does not cover
        if (flags & SMC_FLAG_SYSTEMATIC)
            return fail(SMC_EINVAL, "smc_create: SMC_FLAG_CONDITIONAL with SMC_FLAG_SYSTEMATIC (conditional systematic resampling is another algorithm)");
        if (flags & SMC_FLAG_NAN_MISSING) return fail(SMC_EINVAL, "smc_create: SMC_FLAG_CONDITIONAL with SMC_FLAG_NAN_MISSING (no gaps in conditional runs)");
        if (!has_density(model_id))
            return fail(SMC_EINVAL, "smc_create: SMC_FLAG_CONDITIONAL with SMC_MODEL_UCSV_RB (its state rows have no transition density: no backward simulation)");
        if (n_x > PATH_MAX_N) return fail(SMC_EINVAL, "smc_create: SMC_FLAG_CONDITIONAL with n_x > 2^20 (the limit of the backward walk, smc_sample_paths)");
    }
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (ndev == 0) return fail(SMC_EHIP, "smc_create: no HIP device; this library has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(SMC_EINVAL, "smc_create: bad device index");
    HIPCHK(hipSetDevice(device));

    smc_filter_s* h = new smc_filter_s();
    h->model = model_id; h->d = d; h->device = device; h->flags = flags;
    h->geo = g;
    FilterView& v = h->v;
    v.n = n_x; v.seg = seg; v.nseg = (int)nseg; v.npad = nseg * seg; v.ntheta = (int)n_theta; v.seed = seed;
    int p2 = 1;
    while (p2 < v.nseg) p2 <<= 1;
    v.nseg_p2 = p2;
    v.SH = table_shift_extra(v.npad);
    v.want_s2 = 1;
#ifdef SMC_ABLATE
    v.abl = h_abl_tmp;
    if (getenv("SMC_DBG")) {
        if (hipMalloc((void**)&v.dbg, (size_t)v.ntheta * v.nseg * 128) != hipSuccess) v.dbg = nullptr;   // second half: the start-up stamps
        else (void)hipMemset(v.dbg, 0, (size_t)v.ntheta * v.nseg * 128);
    }
#endif
    h->resident_ok = (v.nseg == 1) && !(flags & (SMC_FLAG_NO_RESIDENT | SMC_FLAG_CONDITIONAL));   // (conditional: one launch per step only)
    v.systematic = (flags & SMC_FLAG_SYSTEMATIC) ? 1 : 0;
    v.inv_n = 1.0 / (double)n_x;

    const size_t np = (size_t)v.ntheta * (size_t)v.npad, ns = (size_t)v.ntheta * (size_t)v.nseg, nt = (size_t)v.ntheta;
#define TRY(expr)                                       \
    do {                                                \
        hipError_t _e = (expr);                         \
        if (_e != hipSuccess) {                         \
            std::string m = hipGetErrorString(_e);      \
            smc_destroy(h);                             \
            return fail(SMC_ENOMEM, "smc_create: " #expr ": " + m); \
        }                                               \
    } while (0)
    Bundle bun;   // filled from the cache once the sizes are known (below); fresh resources otherwise
    {   // every array the handle always owns, in ONE device allocation (smc_create + smc_destroy of a 1024-particle filter: 0.63 ->
        // 0.55 ms; thirty-odd hipMalloc / hipFree calls cost more than the filter's hundred steps)
        const bool gtab = v.nseg_p2 > 2 * g.threads;   // more than twice as many segments as a workgroup has threads: the segment table is built once per step (k_table)
        OffsetPlan slab;
        const size_t o_params = slab.take(nt * sizeof(*h->d_params)), o_stream = slab.take(nt * sizeof(*h->d_stream)), o_perm = slab.take(nt * sizeof(*h->d_perm)),
                     o_ztmp = slab.take(nt * 8);
        size_t o_x[2], o_C[2], o_k[2], o_S[2], o_hi[2], o_lo[2];
        for (int b = 0; b < 2; ++b) {
            o_x[b] = slab.take(np * (size_t)d * 8); o_C[b] = slab.take(np * 8);
            o_k[b] = slab.take(ns * 8); o_S[b] = slab.take(ns * 8); o_hi[b] = slab.take(ns * 8); o_lo[b] = slab.take(ns * 8);
        }
        const size_t o_anc = (flags & SMC_FLAG_ANCESTORS) ? slab.take(np * 4) : 0;
        const size_t o_logZ = slab.take(nt * 8), o_lm = slab.take(nt * 8), o_es = slab.take(nt * 8), o_K = slab.take(nt * 8), o_D = slab.take(nt * 8);
        const size_t o_tD = gtab ? slab.take(nt * (size_t)v.nseg_p2 * 8) : 0, o_tsh = gtab ? slab.take(nt * (size_t)v.nseg_p2 * 4) : 0;
        if (bundle_cache().take(device, slab.bytes, 4 * nt * 8, bun)) {
            h->d_slab = std::move(bun.slab); h->stream = bun.stream; h->ev0 = bun.ev0; h->ev1 = bun.ev1;
            h->h_pin = std::move(bun.pin);
            h->d_y = std::move(bun.d_y);
            h->d_recs = std::move(bun.d_recs);   // (how many steps it holds for THIS handle's n_theta: ensure_recs)
            if (bun.h_params.bytes() >= nt * sizeof(Params)) h->h_params = std::move(bun.h_params);   // (else freed with bun)
        } else {
            TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
            TRY(hipEventCreate(&h->ev0));
            TRY(hipEventCreate(&h->ev1));
            TRY(h->d_slab.grow(slab.bytes));
        }
        TRY(hipMemsetAsync(h->d_slab.as<char>(), 0, slab.bytes, h->stream));
        char* base = h->d_slab.as<char>();
        h->d_params = (decltype(h->d_params))(base + o_params); h->d_stream = (decltype(h->d_stream))(base + o_stream);
        h->d_perm = (decltype(h->d_perm))(base + o_perm); h->d_logZ_tmp = (double*)(base + o_ztmp);
        for (int b = 0; b < 2; ++b) {
            v.x[b] = (double*)(base + o_x[b]); v.C[b] = (uint64_t*)(base + o_C[b]);
            v.segk[b] = (double*)(base + o_k[b]); v.segS[b] = (uint64_t*)(base + o_S[b]);
            v.segS2hi[b] = (uint64_t*)(base + o_hi[b]); v.segS2lo[b] = (uint64_t*)(base + o_lo[b]);
        }
        if (flags & SMC_FLAG_ANCESTORS) v.anc = (decltype(v.anc))(base + o_anc);
        v.logZ = (double*)(base + o_logZ); v.last_logmu = (double*)(base + o_lm); v.last_ess = (double*)(base + o_es);
        v.last_K = (double*)(base + o_K); v.last_D = (uint64_t*)(base + o_D);
        if (gtab) { v.tabD = (uint64_t*)(base + o_tD); v.tabsh = (int*)(base + o_tsh); }
    }
    TRY(h->h_pin.grow(4 * nt * 8));   // (a recycled one holds at least that: take)
    memset(h->h_pin.as<double>(), 0, 4 * nt * 8);
    v.host_out = h->h_pin.as<double>();
    std::vector<uint32_t> st(nt);
    for (size_t m = 0; m < nt; ++m) st[m] = (uint32_t)m;
    TRY(hipMemcpyAsync(h->d_stream, st.data(), nt * 4, hipMemcpyHostToDevice, h->stream));
    TRY(hipStreamSynchronize(h->stream));
#undef TRY
    h->hot.stream0 = 0u;
    h->hot.stream_ok = true;
    if (const char* e = getenv("SMC_STEP_BY_VALUE")) h->hot.allow = atoi(e) != 0;   // 0: every step launch through the pointers
    v.params = h->d_params;
    v.stream = h->d_stream;
    *out = h;
    return SMC_OK;
}

extern "C" int smc_destroy(smc_handle h) {
    if (!h) return SMC_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
#ifdef SMC_ABLATE
    abl_report(h);
#endif
    // a whole handle (smc_create's TRY comes here with half of one) offers the cache its bundle (the stream is idle: synchronised
    // above); one the cache refuses is freed here, and everything else the handle owns with the handle
    bool kept = false;
    if (h->d_slab && h->h_pin && h->stream && h->ev0 && h->ev1) {
        Bundle bun{h->device, std::move(h->d_slab), std::move(h->h_pin), h->stream, h->ev0, h->ev1, std::move(h->d_y), std::move(h->d_recs),
                   std::move(h->h_params)};
        kept = bundle_cache().give(bun);
    }
    if (!kept) {
        if (h->ev0) (void)hipEventDestroy(h->ev0);
        if (h->ev1) (void)hipEventDestroy(h->ev1);
        if (h->stream) (void)hipStreamDestroy(h->stream);
    }
    delete h;
    return SMC_OK;
}

// the proposal row of filter m from its parameter row (and, AFFINE, from the stored row): smc_spec.h "proposals"
static void fill_proposal(smc_handle h, int m) {
    const Params& P = h->h_params.as<Params>()[m];
    double* q = h->h_prop.as<PropRow>()[m].p;
    for (int k = 0; k < NPARAM; ++k) q[k] = 0.0;
    if (h->v.prop_kind == PROP_AFFINE)
        for (int k = 0; k < PROP_NPAR; ++k) q[k] = h->prop_par[(size_t)m * PROP_NPAR + k];
    derive_proposal(h->model, h->v.prop_kind, P.raw, P.der, q);
}

extern "C" int smc_set_params(smc_handle h, const double* raw) {
    if (!h || !raw) return fail(SMC_EINVAL, "smc_set_params: NULL argument");
    HIPCHK(hipSetDevice(h->device));
    const int nraw = model_nraw_rt(h->model);
    // the rows are derived into a pinned twin and copied from there: the call does not wait for the device (what follows on the
    // handle is ordered behind the copy); a previous copy out of the twin has completed once the stream is idle
    if (!h->h_params) HIPCHK(h->h_params.grow((size_t)h->v.ntheta * sizeof(Params)));
    else HIPCHK(hipStreamSynchronize(h->stream));
    Params* P = h->h_params.as<Params>();
    for (int m = 0; m < h->v.ntheta; ++m) {
        params_from_raw(h->model, raw + (size_t)m * nraw, P[m]);
        if (h->v.prop_kind) fill_proposal(h, m);
    }
    h->win.k = 0;   // an uncommitted window belongs to the previous rows (include/smc_hip.h "pending window")
    HIPCHK(hipMemcpyAsync(h->d_params, P, (size_t)h->v.ntheta * sizeof(Params), hipMemcpyHostToDevice, h->stream));
    h->hot.prm0 = P[0];
    h->hot.prm_ok = true;
    if (h->v.prop_kind)   // a guided handle: the proposal rows follow the parameter rows
        HIPCHK(hipMemcpyAsync(h->d_prop.as<PropRow>(), h->h_prop.as<PropRow>(), (size_t)h->v.ntheta * sizeof(PropRow), hipMemcpyHostToDevice, h->stream));
    h->have_params = true;
    return SMC_OK;
}

extern "C" int smc_set_proposal(smc_handle h, int kind, const double* par) {
    if (!h) return fail(SMC_EINVAL, "smc_set_proposal: NULL handle");
    if (kind != PROP_NONE && kind != PROP_AFFINE && kind != PROP_OPTIMAL) return fail(SMC_EINVAL, "smc_set_proposal: unknown kind");
    if (conditional(h) && kind != PROP_NONE)
        return fail(SMC_EINVAL, "smc_set_proposal: the handle is conditional (SMC_FLAG_CONDITIONAL): guided conditional filters are not covered");
    if (h->model == MODEL_UCSV_RB && kind != PROP_NONE)
        return fail(SMC_EINVAL, "smc_set_proposal: SMC_MODEL_UCSV_RB takes no proposal (its step already conditions on y: the trend is integrated out)");
    if (!proposal_supported(h->model, kind)) return fail(SMC_EINVAL, "smc_set_proposal: this model family has no proposal of that kind");
    if ((kind == PROP_AFFINE) != (par != nullptr)) return fail(SMC_EINVAL, "smc_set_proposal: rows are given with SMC_PROP_AFFINE and only then");
    if (kind == PROP_AFFINE)
        for (int m = 0; m < h->v.ntheta; ++m)
            if (!affine_row_ok(par + (size_t)m * PROP_NPAR)) return fail(SMC_EINVAL, "smc_set_proposal: rows must be finite with s2 > 0");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t nt = (size_t)h->v.ntheta;
    if (kind != PROP_NONE) {
        HIPCHK(h->d_prop.grow(nt * sizeof(PropRow)));
        HIPCHK(h->h_prop.grow(nt * sizeof(PropRow)));
    }
    if (kind == PROP_AFFINE) h->prop_par.assign(par, par + nt * PROP_NPAR);
    else h->prop_par.clear();
    h->v.prop_kind = kind;
    h->v.prop = kind != PROP_NONE ? h->d_prop.as<PropRow>() : nullptr;
    h->win.k = 0;   // an uncommitted window belongs to the previous proposal
    if (kind == PROP_NONE) return SMC_OK;
    // the rows on the device.  The parameter rows they derive from are read back first: a proposal handle of the device PMMH had
    // them written there (k_pmmh_propose), not through the pinned twin.  Without parameters yet: the rows as given, the
    // constants follow with smc_set_params / the device PMMH
    if (!h->h_params) {
        HIPCHK(h->h_params.grow(nt * sizeof(Params)));
        memset(h->h_params.as<Params>(), 0, nt * sizeof(Params));
    }
    if (h->have_params) HIPCHK(hipMemcpy(h->h_params.as<Params>(), h->d_params, nt * sizeof(Params), hipMemcpyDeviceToHost));
    for (int m = 0; m < h->v.ntheta; ++m) fill_proposal(h, m);
    HIPCHK(hipMemcpyAsync(h->d_prop.as<PropRow>(), h->h_prop.as<PropRow>(), nt * sizeof(PropRow), hipMemcpyHostToDevice, h->stream));
    return SMC_OK;
}

extern "C" int smc_set_streams(smc_handle h, const uint32_t* s) {
    if (!h || !s) return fail(SMC_EINVAL, "smc_set_streams: NULL argument");
    HIPCHK(hipSetDevice(h->device));
    h->win.k = 0;   // an uncommitted window belongs to the previous stream ids
    HIPCHK(hipMemcpyAsync(h->d_stream, s, (size_t)h->v.ntheta * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->hot.stream0 = s[0];
    h->hot.stream_ok = true;
    h->brk_count = 0;    // cached break points belong to the old stream ids
    return SMC_OK;
}

extern "C" int smc_step_by_value(smc_handle h, int* by_value) {
    if (!h || !by_value) return fail(SMC_EINVAL, "smc_step_by_value: NULL argument");
    *by_value = hot_legal(h) && !h->skip.on ? 1 : 0;
    return SMC_OK;
}

extern "C" int smc_get_launch_geometry(smc_handle h, int* threads, int* np, int* resident_np) {
    if (!h) return fail(SMC_EINVAL, "smc_get_launch_geometry: NULL handle");
    if (threads) *threads = h->geo.threads;
    if (np) *np = h->geo.np;
    if (resident_np) {
        const int r = smc::resident_np(h->v);   // the environment as the launch would read it now
        *resident_np = (r == 1 || r == 2 || r == 4) ? r : 0;   // (any other value selects what 0 does)
    }
    return SMC_OK;
}

extern "C" int smc_reseed(smc_handle h, uint64_t seed) {
    if (!h) return fail(SMC_EINVAL, "smc_reseed: NULL handle");
    h->v.seed = seed;
    h->win.k = 0;        // an uncommitted window belongs to the old seed
    h->brk_count = 0;    // cached break points belong to the old seed
    return SMC_OK;
}

// the blocks of the whole-series calls hold T steps (old block first, behind an idle stream; almost always a no-op)
static int ensure_steps(smc_handle h, DevBlock& b, size_t bytes) {
    if (bytes > b.bytes()) {
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(b.grow(bytes));
    }
    return SMC_OK;
}
int ensure_y(smc_handle h, int64_t T) { return ensure_steps(h, h->d_y, (size_t)T * 8); }
int ensure_recs(smc_handle h, int64_t T) { return ensure_steps(h, h->d_recs, (size_t)T * (size_t)h->v.ntheta * sizeof(StepRec)); }

// Close the timed region (ev1) and hand the requested per-filter result vectors to the caller from the
// pinned mirror (FilterView::host_out): ONE stream synchronisation, no copy commands.
int finish_elapsed(smc_handle h, double* logZ, double* logmu, double* ess) {
    const size_t nt = (size_t)h->v.ntheta;
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));   // the emitting kernel stored the results in the pinned mirror itself
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    h->last_ms = ms;
    const double* pin = h->h_pin.as<double>();
    if (logZ) memcpy(logZ, pin, nt * 8);
    if (logmu) memcpy(logmu, pin + nt, nt * 8);
    if (ess) memcpy(ess, pin + 2 * nt, nt * 8);
    return SMC_OK;
}

// Step API (smc_init / smc_step): the emitting kernel stores a ticket behind its three values (host_emit); the host spins on the
// pinned words - no event records, no stream synchronisation (32 -> 12 us per call for a filter of 1024 particles).  A ticket
// that does not show up within 50 ms is looked for once more after a real synchronisation (a faulted launch reports there).
static int wait_ticket(smc_handle h, uint32_t seq, double* logmu, double* ess) {
    const size_t nt = (size_t)h->v.ntheta;
    const double* pin = h->h_pin.as<double>();
    const volatile double* tk = pin + 3 * nt;
    const double want = (double)seq;
    const auto t0 = std::chrono::steady_clock::now();
    bool synced = false;
    unsigned spins = 0;
    for (size_t th = 0; th < nt;) {
        if (tk[th] == want) { ++th; continue; }
        if ((++spins & 0x3ffu) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(50)) {
            if (synced) return fail(SMC_EHIP, "step API: the launch completed without its result ticket");
            HIPCHK(hipStreamSynchronize(h->stream));
            synced = true;
        }
        __builtin_ia32_pause();
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    if (logmu) memcpy(logmu, pin + nt, nt * 8);
    if (ess) memcpy(ess, pin + 2 * nt, nt * 8);
    h->last_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();   // host clock of the wait
    return SMC_OK;
}

// the next ticket of the step API - or 0: batches of more than 64 filters synchronise the stream instead (every filter's emitting
// thread releases its values to the host by itself: 4096 of them take 360 us per step against 74 for events + synchronisation;
// measured equal at 512 filters, scripts/dbg/step_latency_batch.py)
static uint32_t step_ticket(smc_handle h) {
    if (h->v.ntheta > 64) return 0;
    return ++h->seq ? h->seq : ++h->seq;
}
int emit_if_needed(smc_handle h) {
    if (!h->emitted) {
        HIPCHK(do_finalize(h, h->t == 1 ? 1 : 0, h->t - 1));
        h->emitted = true;
    }
    return SMC_OK;
}

// bootstrap_filter(N, y, model)   particles.jl:87-105
extern "C" int smc_init(smc_handle h, double y1, double* logmu) {
    if (!h) return fail(SMC_EINVAL, "smc_init: NULL handle");
    if (!h->have_params) return fail(SMC_ESTATE, "smc_init: smc_set_params has not been called");
    if (conditional(h) && !h->cond.d_xref)
        return fail(SMC_ESTATE, "smc_init: the handle is conditional (SMC_FLAG_CONDITIONAL) and has no reference (smc_set_reference)");
    h->win.k = 0;   // an uncommitted window is dropped
    HIPCHK(hipSetDevice(h->device));
    h->v.y = nullptr; h->v.trace_logmu = nullptr; h->v.trace_ess = nullptr;
    h->cur = 0;
    const bool own = h->v.nseg == 1;   // one workgroup owns the filter: it emits (logmu, ess) itself
    const uint32_t seq = step_ticket(h);
    if (!seq) HIPCHK(hipEventRecord(h->ev0, h->stream));
    h->v.emit_now = own ? 1 : 0;
    h->v.host_seq = seq;
    hipError_t le = do_init(h, y1);
    h->v.emit_now = 0;
    if (le == hipSuccess) { h->t = 1; h->inited = true; h->emitted = own; }
    const int rc = le == hipSuccess ? emit_if_needed(h) : SMC_OK;
    h->v.host_seq = 0;
    HIPCHK(le);
    if (rc) return rc;
    if (history_armed(h)) {   // smc_init restarts the record
        h->hist.len = 0;
        h->hist.walk_M = 0;   // (the last walk's indices belonged to the record this run overwrites)
        if (const int hr = history_append(h)) return hr;
    }
    return seq ? wait_ticket(h, seq, logmu, nullptr) : finish_elapsed(h, nullptr, logmu, nullptr);
}

// bootstrap_filter!(x, w, y, model)   particles.jl:107-129
extern "C" int smc_step(smc_handle h, double y_t, double* logmu, double* ess) {
    if (!h) return fail(SMC_EINVAL, "smc_step: NULL handle");
    if (!h->inited) return fail(SMC_ESTATE, "smc_step: call smc_init (bootstrap_filter) first");
    if (history_armed(h) && h->hist.len >= h->hist.cap) return fail(SMC_ESTATE, "smc_step: the record is full (smc_history_begin's T_cap)");
    if (conditional(h) && (!h->cond.d_xref || (int64_t)h->t >= h->cond.T))
        return fail(SMC_ESTATE, "smc_step: the reference of the conditional handle ends before this step (smc_set_reference's T)");
    h->win.k = 0;   // an uncommitted window is dropped
    HIPCHK(hipSetDevice(h->device));
    h->v.y = nullptr; h->v.trace_logmu = nullptr; h->v.trace_ess = nullptr;
    int rc = emit_if_needed(h);   // (a pending emission of the previous step goes first, without a ticket)
    if (rc) return rc;
    HIPCHK(ensure_breaks(h, h->t, h->t + 64));   // step API: 64 steps of break points at a time
    const bool own = h->v.nseg == 1;
    const uint32_t seq = step_ticket(h);
    if (!seq) HIPCHK(hipEventRecord(h->ev0, h->stream));
    h->v.emit_now = own ? 1 : 0;
    h->v.host_seq = seq;
    hipError_t le = do_step(h, h->t, 0, y_t);
    h->v.emit_now = 0;
    if (le == hipSuccess) { h->cur ^= 1; h->t += 1; h->emitted = own; rc = emit_if_needed(h); }
    h->v.host_seq = 0;
    HIPCHK(le);
    if (rc) return rc;
    if (history_armed(h) && (rc = history_append(h))) return rc;
    return seq ? wait_ticket(h, seq, logmu, ess) : finish_elapsed(h, nullptr, logmu, ess);
}

// ---- k steps in one launch (the online sampler's window) ---------------------------------------------------------
constexpr int WIN_MAX = 64;
static int launch_window_steps(smc_handle h, int k) {
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    HIPCHK(do_window(h, k, h->cur ^ 1));
    return SMC_OK;
}
extern "C" int smc_step_window(smc_handle h, const double* y, int k, double* logmu, double* ess) {
    if (!h || !y) return fail(SMC_EINVAL, "smc_step_window: NULL argument");
    if (conditional(h)) return cond_refuse("smc_step_window");
    if (!h->inited) return fail(SMC_ESTATE, "smc_step_window: call smc_init (bootstrap_filter) first");
    if (history_armed(h)) return history_refuse("smc_step_window");
    if (k < 1 || k > WIN_MAX) return fail(SMC_EINVAL, "smc_step_window: 1 <= k <= 64");
    if (h->v.nseg != 1 || !resident_supported(h->model, h->v.seg))
        return fail(SMC_EINVAL, "smc_step_window: needs filters that fit the LDS-resident kernel (one segment); use smc_step");
    HIPCHK(hipSetDevice(h->device));
    int rc = emit_if_needed(h);
    if (rc) return rc;
    if ((rc = ensure_y(h, WIN_MAX))) return rc;
    if ((rc = ensure_recs(h, WIN_MAX))) return rc;
    const size_t nt = (size_t)h->v.ntheta;
    HIPCHK(h->win.h_out.grow(2 * (size_t)WIN_MAX * nt * 8));
    const bool summ = summaries_on(h);
    if (summ && h->v.systematic) return fail(SMC_EINVAL, "smc_step_window: per-step summaries need the default (multinomial) resampler");
    if (summ && !summaries_fit_lds(h)) return fail(SMC_EINVAL, "smc_step_window: no LDS left for the summaries of filters this long; fewer levels, or smc_step");
    if (summ && (rc = ensure_summaries(h, WIN_MAX))) return rc;
    h->summ.T = 0;
    h->summ.skip.clear();   // (the skip mask applies to smc_log_likelihood only)
    HIPCHK(hipMemcpyAsync(h->d_y.as<double>(), y, (size_t)k * 8, hipMemcpyHostToDevice, h->stream));
    h->v.y = h->d_y.as<double>();
    if (summ) view_summaries(h);
    h->win.gap = series_has_gap(h, y, k);
    rc = launch_window_steps(h, k);
    h->v.y = nullptr;
    h->v.sum_np = h->v.sum_mom = 0; h->v.sum_q = h->v.sum_m = nullptr;
    if (rc) return rc;
    if (summ) h->summ.T = k;
    if ((rc = finish_elapsed(h))) return rc;
    if (logmu) memcpy(logmu, h->win.h_out.as<double>(), (size_t)k * nt * 8);
    if (ess) memcpy(ess, h->win.h_out.as<double>() + (size_t)k * nt, (size_t)k * nt * 8);
    h->win.k = k;
    return SMC_OK;
}
extern "C" int smc_step_commit(smc_handle h, int j) {
    if (!h) return fail(SMC_EINVAL, "smc_step_commit: NULL handle");
    if (conditional(h)) return cond_refuse("smc_step_commit");
    if (history_armed(h)) return history_refuse("smc_step_commit");
    if (h->win.k == 0) return fail(SMC_ESTATE, "smc_step_commit: no window pending (smc_step_window)");
    if (j < 0 || j > h->win.k) return fail(SMC_EINVAL, "smc_step_commit: 0 <= j <= steps of the window");
    HIPCHK(hipSetDevice(h->device));
    const int k = h->win.k;
    h->win.k = 0;
    if (j == 0) return SMC_OK;            // nothing kept: the filters stand where they stood before the window
    if (j < k) {                          // keep a prefix: the same j steps again (counter-based random numbers: the same bits)
        h->v.y = h->d_y.as<double>();
        int rc = launch_window_steps(h, j);
        h->v.y = nullptr;
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_commit, dim3((unsigned)((h->v.ntheta + 127) / 128)), dim3(128), 0, h->stream, h->v, j, h->d_recs.as<StepRec>());
    HIPCHK(hipGetLastError());
    h->cur ^= 1; h->t += (uint32_t)j; h->emitted = true;
    return SMC_OK;      // no wait: whatever the caller does next with this handle is ordered behind on its stream
}

// Filters smc_log_likelihood leaves out (logZ = -inf): the proposals outside the prior's support, for which the
// reference never calls log_likelihood (smc_samplers.jl:116).  NULL: run every filter again.
extern "C" int smc_set_skip(smc_handle h, const uint8_t* skip) {
    if (!h) return fail(SMC_EINVAL, "smc_set_skip: NULL handle");
    HIPCHK(hipSetDevice(h->device));
    if (!skip) { h->skip.on = false; h->skip.h_mask.clear(); return SMC_OK; }
    const int nt = h->v.ntheta;
    HIPCHK(h->skip.d_mask.grow((size_t)nt));
    HIPCHK(h->skip.d_order.grow(((size_t)nt + 1) * 4));
    std::vector<int32_t> ord((size_t)nt + 1);
    int na = 0, ns = 0;
    for (int m = 0; m < nt; ++m) {
        if (skip[m]) ord[(size_t)nt - 1 - ns++] = m;
        else ord[(size_t)na++] = m;
    }
    ord[(size_t)nt] = na;
    HIPCHK(hipMemcpyAsync(h->skip.d_mask.as<unsigned char>(), skip, (size_t)nt, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->skip.d_order.as<int32_t>(), ord.data(), ord.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->skip.h_mask.assign(skip, skip + nt);
    h->skip.on = true;
    return SMC_OK;
}

extern "C" int smc_get_logZ(smc_handle h, double* logZ, double* ess) {
    if (!h) return fail(SMC_EINVAL, "smc_get_logZ: NULL handle");
    if (!h->inited) return fail(SMC_ESTATE, "smc_get_logZ: filter not initialised");
    HIPCHK(hipSetDevice(h->device));
    int rc = emit_if_needed(h);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    if (logZ) HIPCHK(hipMemcpy(logZ, h->v.logZ, (size_t)h->v.ntheta * 8, hipMemcpyDeviceToHost));
    if (ess) HIPCHK(hipMemcpy(ess, h->v.last_ess, (size_t)h->v.ntheta * 8, hipMemcpyDeviceToHost));
    return SMC_OK;
}

extern "C" int smc_get_flags(smc_handle h, uint32_t* flags) {
    if (!h || !flags) return fail(SMC_EINVAL, "smc_get_flags: NULL argument");
    *flags = h->flags;
    return SMC_OK;
}

extern "C" int smc_get_geometry(smc_handle h, int* seg, int* nseg, int* d, int* resident) {
    if (!h) return fail(SMC_EINVAL, "smc_get_geometry: NULL handle");
    if (seg) *seg = h->v.seg;
    if (nseg) *nseg = h->v.nseg;
    if (d) *d = h->d;
    if (resident) *resident = (h->resident_ok && resident_supported(h->model, h->v.seg)) ? 1 : 0;
    return SMC_OK;
}

extern "C" int smc_last_elapsed_ms(smc_handle h, double* ms) {
    if (!h || !ms) return fail(SMC_EINVAL, "smc_last_elapsed_ms: NULL argument");
    *ms = h->last_ms;
    return SMC_OK;
}

extern "C" int smc_synchronize(smc_handle h) {
    if (!h) return fail(SMC_EINVAL, "smc_synchronize: NULL handle");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    return SMC_OK;
}

#ifdef SMC_ABLATE
// profiling builds: what the stamps of the LAST launches say (FilterView::dbg), printed when the handle goes
static void abl_report(smc_filter_s* h) {
    if (h->v.dbg && h->v.nseg == 1) {   // placement and lifetime of the workgroups of the LAST k_resident launch
        const size_t nwg = (size_t)h->v.ntheta;
        std::vector<unsigned long long> st(nwg * 8);
        (void)hipMemcpy(st.data(), h->v.dbg, nwg * 64, hipMemcpyDeviceToHost);
        unsigned long long t0 = ~0ull, t1 = 0;
        std::map<unsigned long long, std::vector<size_t>> bycu;
        size_t nact = 0;
        for (size_t w = 0; w < nwg; ++w) {
            if (!st[w * 8 + 1]) continue;
            ++nact;
            if (st[w * 8] < t0) t0 = st[w * 8];
            if (st[w * 8 + 1] > t1) t1 = st[w * 8 + 1];
            const unsigned long long hw = st[w * 8 + 2];
            const unsigned long long key = ((hw >> 32) & 0xf) << 16 | ((hw >> 8) & 0xff);   // (xcc, se/sh/cu)
            bycu[key].push_back(w);
        }
        int hist[9] = {0};
        double life[9] = {0};
        for (auto& kv : bycu) {
            const size_t c = kv.second.size() < 8 ? kv.second.size() : 8;
            hist[c]++;
            for (size_t w : kv.second) life[c] += (double)(st[w * 8 + 1] - st[w * 8]) * 0.01;
        }
        fprintf(stderr, "[dbg] k_resident: %zu workgroups ran on %zu CUs, span %.1f us;", nact, bycu.size(), (double)(t1 - t0) * 0.01);
        for (int c = 1; c <= 8; ++c)
            if (hist[c]) fprintf(stderr, "  %d CUs with %d workgroups (mean life %.1f us)", hist[c], c, life[c] / (hist[c] * c));
        fprintf(stderr, "\n");
        {   // start times of the workgroups sharing a CU: simultaneous or one after the other?
            int shown = 0;
            for (auto& kv : bycu) {
                if (shown++ >= 4) break;
                fprintf(stderr, "[dbg]   cu %05llx:", kv.first);
                for (size_t w : kv.second) fprintf(stderr, " wg %zu [%.1f, %.1f]", w, (double)(st[w * 8] - t0) * 0.01, (double)(st[w * 8 + 1] - t0) * 0.01);
                fprintf(stderr, "\n");
            }
        }
        (void)hipFree(h->v.dbg);
        h->v.dbg = nullptr;
    }
    if (h->v.dbg) {   // phase profile of the LAST k_step launch: mean over workgroups, in microseconds
        const size_t nwg = (size_t)h->v.ntheta * h->v.nseg;
        std::vector<unsigned long long> st(nwg * 8);
        (void)hipMemcpy(st.data(), h->v.dbg, nwg * 64, hipMemcpyDeviceToHost);
        unsigned long long t0 = ~0ull, t7 = 0;
        double ph[8] = {0};
        for (size_t w = 0; w < nwg; ++w) {
            if (st[w * 8] < t0) t0 = st[w * 8];
            if (st[w * 8 + 7] > t7) t7 = st[w * 8 + 7];
            for (int k = 1; k < 8; ++k) ph[k] += (double)(st[w * 8 + k] - st[w * 8 + k - 1]) * 0.01;
        }
        {   // start-up latency of the LAST k_step launch: entry of a workgroup's first wave -> its first pick numbers drawn
            std::vector<unsigned long long> sd(nwg * 8);
            (void)hipMemcpy(sd.data(), h->v.dbg + nwg * 8, nwg * 64, hipMemcpyDeviceToHost);
            if (sd[0] != 0 && sd[1] != 0) {   // (systematic launches draw no pick numbers: no stamp)
                double sum = 0, mn = 1e30, mx = 0;
                std::vector<double> all(nwg);
                for (size_t w = 0; w < nwg; ++w) {
                    const double us = (double)(sd[w * 8] - sd[w * 8 + 1]) * 0.01;
                    all[w] = us; sum += us; mn = std::min(mn, us); mx = std::max(mx, us);
                }
                std::sort(all.begin(), all.end());
                fprintf(stderr, "[dbg] k_step start-up, entry -> first pick numbers drawn, over %zu workgroups (us, 10 ns clock): mean %.3f min %.3f "
                                "median %.3f 90%% %.3f max %.3f\n", nwg, sum / nwg, mn, all[nwg / 2], all[(size_t)((nwg - 1) * 0.9)], mx);
            }
        }
        double start_spread = 0, life = 0;
        for (size_t w = 0; w < nwg; ++w) { start_spread += (double)(st[w * 8] - t0) * 0.01; life += (double)(st[w * 8 + 7] - st[w * 8]) * 0.01; }
        fprintf(stderr, "[dbg] k_step span %.2f us; mean start offset %.2f us; mean WG life %.2f us; phases(us):", (double)(t7 - t0) * 0.01,
                start_spread / nwg, life / nwg);
        const char* nm[8] = {"", "table+picks", "targets+range+lookup", "normals", "T2+stage-write+barrier", "search", "gather+model+store", "epilogue"};
        for (int k = 1; k < 8; ++k) fprintf(stderr, " %s=%.2f", nm[k], ph[k] / nwg);
        fprintf(stderr, "\n");
        {   // the slowest workgroups: where do they lose time, and where do they sit (XCD = launch index % 8)
            std::vector<size_t> idx(nwg);
            for (size_t w = 0; w < nwg; ++w) idx[w] = w;
            std::sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return st[a * 8 + 7] > st[b * 8 + 7]; });
            for (size_t r = 0; r < 6 && r < nwg; ++r) {
                const size_t w = idx[r];
                fprintf(stderr, "[dbg]   late #%zu wg %zu xcd %zu: start %.2f end %.2f phases", r, w, w % 8, (double)(st[w * 8] - t0) * 0.01,
                        (double)(st[w * 8 + 7] - t0) * 0.01);
                for (int k = 1; k < 8; ++k) fprintf(stderr, " %.2f", (double)(st[w * 8 + k] - st[w * 8 + k - 1]) * 0.01);
                fprintf(stderr, "\n");
            }
            double endq[5];
            std::vector<double> ends(nwg);
            for (size_t w = 0; w < nwg; ++w) ends[w] = (double)(st[w * 8 + 7] - t0) * 0.01;
            std::sort(ends.begin(), ends.end());
            const double qs[5] = {0.1, 0.5, 0.9, 0.99, 1.0};
            for (int k = 0; k < 5; ++k) endq[k] = ends[(size_t)((nwg - 1) * qs[k])];
            fprintf(stderr, "[dbg]   end-time quantiles (us) 10%%=%.2f 50%%=%.2f 90%%=%.2f 99%%=%.2f max=%.2f\n", endq[0], endq[1], endq[2], endq[3], endq[4]);
        }
        (void)hipFree(h->v.dbg);
    }
}
#endif
