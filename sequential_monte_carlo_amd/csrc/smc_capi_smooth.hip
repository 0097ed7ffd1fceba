// smc_capi_smooth.hip -- the record of a step-by-step run (smc_history_*) and the backward passes over it.  smc_smooth: the FFBS
// particle smoother, forward filtering by the step kernels as they are, backward smoothing by the all-pairs kernels of
// smc_smooth_kernels.h; smc_smooth_pairs and smc_smooth_quantiles are the same pass with more kept (smooth_run).
// smc_sample_paths and smc_rb_sample_paths (MODEL_UCSV_RB): backward simulation, ONE walk over the record
// (backward_walk: the refusals, the plan of the block, the uploads, the dead scan and the loop over the steps, smc_path_kernels.h)
// that each of the two entry points wraps with the tail of its plan and with what follows the walk (smc_rb_kernels.h).
// The ancestor plane of the record of an SMC_FLAG_ANCESTOR_SAMPLING handle (smc_history_get_ancestors / _put_ancestors) and the two
// launches of smc_ancestor_sweep over it (ancestor_sweep_enqueue, smc_anc_kernels.h; the entry point: smc_capi_cond.hip).
// Specification: smc_spec.h "the smoother", "quantiles of the smoothed state", "backward simulation"; the host twins
// (smc_host_smooth, smc_host_smooth_quantiles, smc_host_sample_paths, smc_host_rb_sample_paths) live in smc_util.hip.
#include "smc_host.h"
#include "smc_smooth_kernels.h"
#include "smc_path_kernels.h"
#include "smc_rb_kernels.h"
#include "smc_anc_kernels.h"

#include <cstring>
#include <vector>

using namespace smc;

int history_refuse(const char* who) {
    return fail(SMC_ESTATE, std::string(who) + ": the handle records its steps (smc_history_begin) and this call would change the state "
                                               "without a recordable step; call smc_history_end first");
}

void history_free(smc_filter_s* h) { h->hist = {}; }   // (a disarmed record: its blocks are freed as they are replaced by empty ones)

static size_t cloud_words(const smc_filter_s* h) { return (size_t)h->v.ntheta * (size_t)h->v.n; }

extern "C" int smc_history_begin(smc_handle h, int64_t T_cap) {
    if (!h) return fail(SMC_EINVAL, "smc_history_begin: NULL handle");
    if (T_cap < 1) return fail(SMC_EINVAL, "smc_history_begin: T_cap must be positive");
    HIPCHK(hipSetDevice(h->device));
    const size_t nw = cloud_words(h), per_step = nw * ((size_t)h->d + 1);
    if (per_step > ((size_t)1 << 60) / 8 / (size_t)T_cap) return fail(SMC_ENOMEM, "smc_history_begin: a record of that many bytes cannot be allocated");
    // an ancestor-sampling handle: the ancestor plane int32 [T_cap][n_theta][n] behind the weights, in the same allocation
    const size_t anc_bytes = ancestor_sampling(h) ? nw * (size_t)T_cap * 4 : 0;
    const size_t bytes = per_step * (size_t)T_cap * 8 + anc_bytes;
    // the new block first: a failed allocation leaves the handle as it was.  Armed before: the new record replaces the old one,
    // which the stream may still read
    if (h->hist.rec && bytes > h->hist.rec.bytes()) HIPCHK(hipStreamSynchronize(h->stream));
    const hipError_t e = h->hist.rec.grow_keep(bytes);
    if (e != hipSuccess) return fail(SMC_ENOMEM, std::string("smc_history_begin: hipMalloc of the record: ") + hipGetErrorString(e));
    h->hist.d_x = h->hist.rec.as<double>();
    h->hist.d_w = h->hist.d_x + nw * (size_t)h->d * (size_t)T_cap;
    h->hist.d_a = anc_bytes ? (int32_t*)(h->hist.d_w + nw * (size_t)T_cap) : nullptr;
    h->hist.cap = T_cap;
    h->hist.len = 0;
    h->hist.walk_M = 0;
    h->hist.armed = true;
    return SMC_OK;
}

extern "C" int smc_history_end(smc_handle h) {
    if (!h) return fail(SMC_EINVAL, "smc_history_end: NULL handle");
    HIPCHK(hipSetDevice(h->device));
    if (h->stream) HIPCHK(hipStreamSynchronize(h->stream));
    history_free(h);
    return SMC_OK;
}

extern "C" int smc_history_len(smc_handle h, int64_t* len) {
    if (!h || !len) return fail(SMC_EINVAL, "smc_history_len: NULL argument");
    *len = h->hist.armed ? h->hist.len : 0;
    return SMC_OK;
}

// the state smc_init / smc_step just left, appended on the handle's stream: a device-to-device copy of x and the dense weights
int history_append(smc_handle h) {
    if (h->hist.len >= h->hist.cap) return fail(SMC_ESTATE, "step API: the record is full (smc_history_begin's T_cap)");
    const FilterView& v = h->v;
    const size_t nw = cloud_words(h), t = (size_t)h->hist.len;
    HIPCHK(hipMemcpy2DAsync(h->hist.d_x + t * nw * (size_t)h->d, (size_t)v.n * 8, v.x[h->cur], (size_t)v.npad * 8, (size_t)v.n * 8,
                            (size_t)h->d * v.ntheta, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(enqueue_dense_weights(h, h->hist.d_w + t * nw));
    if (h->hist.d_a) {   // the ancestor vector of this step; the first step has none: -1
        int32_t* a_t = h->hist.d_a + t * nw;
        if (t == 0) HIPCHK(hipMemsetAsync(a_t, 0xFF, nw * 4, h->stream));
        else HIPCHK(hipMemcpy2DAsync(a_t, (size_t)v.n * 4, v.anc, (size_t)v.npad * 4, (size_t)v.n * 4, (size_t)v.ntheta, hipMemcpyDeviceToDevice, h->stream));
    }
    h->hist.len += 1;
    return SMC_OK;
}

extern "C" int smc_history_get(smc_handle h, int64_t t, double* x, double* w) {
    if (!h) return fail(SMC_EINVAL, "smc_history_get: NULL handle");
    if (!h->hist.armed) return fail(SMC_ESTATE, "smc_history_get: the handle does not record (smc_history_begin)");
    if (t < 0 || t >= h->hist.len) return fail(SMC_EINVAL, "smc_history_get: step out of range");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t nw = cloud_words(h);
    if (x) HIPCHK(hipMemcpy(x, h->hist.d_x + (size_t)t * nw * (size_t)h->d, nw * (size_t)h->d * 8, hipMemcpyDeviceToHost));
    if (w) HIPCHK(hipMemcpy(w, h->hist.d_w + (size_t)t * nw, nw * 8, hipMemcpyDeviceToHost));
    return SMC_OK;
}

// overwrites step t of the record (either part may be NULL): the way clouds that no filter run leaves reach the backward pass
extern "C" int smc_history_put(smc_handle h, int64_t t, const double* x, const double* w) {
    if (!h) return fail(SMC_EINVAL, "smc_history_put: NULL handle");
    if (!h->hist.armed) return fail(SMC_ESTATE, "smc_history_put: the handle does not record (smc_history_begin)");
    if (t < 0 || t >= h->hist.len) return fail(SMC_EINVAL, "smc_history_put: step out of range");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t nw = cloud_words(h);
    if (x) HIPCHK(hipMemcpy(h->hist.d_x + (size_t)t * nw * (size_t)h->d, x, nw * (size_t)h->d * 8, hipMemcpyHostToDevice));
    if (w) HIPCHK(hipMemcpy(h->hist.d_w + (size_t)t * nw, w, nw * 8, hipMemcpyHostToDevice));
    return SMC_OK;
}

// the ancestor plane of the record (SMC_FLAG_ANCESTOR_SAMPLING): row t as smc_get_state gave the ancestors after step t
static int need_ancestor_plane(smc_handle h, const char* who, int64_t t) {
    if (!h) return fail(SMC_EINVAL, std::string(who) + ": NULL handle");
    if (!ancestor_sampling(h)) return fail(SMC_ESTATE, std::string(who) + ": the handle was not created with SMC_FLAG_ANCESTOR_SAMPLING");
    if (!h->hist.armed || !h->hist.d_a) return fail(SMC_ESTATE, std::string(who) + ": the handle does not record (smc_history_begin)");
    if (t < 0 || t >= h->hist.len) return fail(SMC_EINVAL, std::string(who) + ": step out of range");
    return SMC_OK;
}

extern "C" int smc_history_get_ancestors(smc_handle h, int64_t t, int32_t* a) {
    const int rc = need_ancestor_plane(h, "smc_history_get_ancestors", t);
    if (rc) return rc;
    if (!a) return fail(SMC_EINVAL, "smc_history_get_ancestors: NULL argument");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t nw = cloud_words(h);
    HIPCHK(hipMemcpy(a, h->hist.d_a + (size_t)t * nw, nw * 4, hipMemcpyDeviceToHost));
    return SMC_OK;
}

extern "C" int smc_history_put_ancestors(smc_handle h, int64_t t, const int32_t* a) {
    const int rc = need_ancestor_plane(h, "smc_history_put_ancestors", t);
    if (rc) return rc;
    if (!a) return fail(SMC_EINVAL, "smc_history_put_ancestors: NULL argument");
    const size_t nw = cloud_words(h);
    for (size_t i = 0; i < nw; ++i)
        if (a[i] < 0 || (int64_t)a[i] >= h->v.n)
            return fail(SMC_EINVAL, "smc_history_put_ancestors: entry " + std::to_string(i) + " is not a particle (outside [0, n_x))");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(h->hist.d_a + (size_t)t * nw, a, nw * 4, hipMemcpyHostToDevice));
    return SMC_OK;
}

// ---- predictive checks over the record (smc_spec.h "predictive checks") ----------------------------------------------------------
// Row t is the row of the cloud recorded at step t for y[t]: smc_get_predictive's kernels over the dense record, in one launch.
extern "C" int smc_predictive(smc_handle h, const double* y, int64_t T, double* pit, double* obs_mean, double* obs_var) {
    if (!h || !y) return fail(SMC_EINVAL, "smc_predictive: NULL argument");
    int rc = predictive_refuse(h, "smc_predictive");
    if (rc) return rc;
    if (!h->hist.armed || h->hist.len < 1) return fail(SMC_ESTATE, "smc_predictive: nothing is recorded (smc_history_begin, then smc_init / smc_step)");
    if (T != h->hist.len)
        return fail(SMC_EINVAL, "smc_predictive: T = " + std::to_string(T) + " observations for " + std::to_string(h->hist.len) + " recorded steps");
    HIPCHK(hipSetDevice(h->device));
    const int64_t n = h->v.n, nt = h->v.ntheta;
    return predictive_run(h, "smc_predictive", h->hist.d_x, (int64_t)h->d * nt * n, nt * n, n, T, y, 0.0, pit, obs_mean, obs_var);
}

// ---- the backward pass ---------------------------------------------------------------------------------------------------
namespace {
// the rows the steps ran with, as the device holds them (the PMMH kernels write them there), and their constants as smooth_row
// derives them for the family `model`; who / what: the caller's name and its wording for a row that is refused
int fetch_rows(smc_handle h, int model, const char* who, const char* what, std::vector<SmoothRow>& rows) {
    const size_t nt = (size_t)h->v.ntheta;
    std::vector<Params> prm(nt);
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(prm.data(), h->d_params, nt * sizeof(Params), hipMemcpyDeviceToHost));
    rows.resize(nt);
    for (size_t m = 0; m < nt; ++m)
        if (!smooth_row(model, prm[m].raw, rows[m]))
            return fail(SMC_EINVAL, std::string(who) + ": " + what + " of filter " + std::to_string(m) + " is not a positive finite number");
    return SMC_OK;
}

struct SmoothPlan {
    int nchunk;
    size_t o_pmax, o_part, o_logD, o_rmax, o_mom, o_rows, o_dead, bytes;   // offsets into hist.d_tmp, in bytes
};
SmoothPlan plan_of(const smc_filter_s* h, int64_t T) {
    SmoothPlan p{};
    const size_t nw = cloud_words(h), nt = (size_t)h->v.ntheta;
    p.nchunk = (int)((h->v.n + SMOOTH_CH - 1) / SMOOTH_CH);
    OffsetPlan o;
    p.o_pmax = o.take((size_t)p.nchunk * nw * 8);
    p.o_part = o.take((size_t)p.nchunk * nw * 8);
    p.o_logD = o.take(nw * 8);
    p.o_rmax = o.take(nw * 8);
    p.o_mom = o.take((size_t)T * nt * (size_t)p.nchunk * 8);
    p.o_rows = o.take(nt * sizeof(SmoothRow));
    p.o_dead = o.take(nt * sizeof(int));
    p.bytes = o.bytes;
    return p;
}

template <int MODEL, int PASS>
hipError_t launch_pairs(const SmoothArgs& a, int threads, hipStream_t s) {
    const dim3 grid((unsigned)((a.n + threads - 1) / threads), (unsigned)a.ntheta, (unsigned)a.nchunk);
    hipLaunchKernelGGL((k_smooth_pairs<MODEL, PASS>), grid, dim3(threads), 0, s, a);
    return hipGetLastError();
}
// cross_t (smc_smooth_pairs): PASS 3 in PASS 2's place (a2.part is then its 1 + 2 d planes), plane 0 through k_smooth_finish as ever,
// the others into cross_t, resid_t
template <int MODEL>
hipError_t backward_step(const SmoothArgs& a01, const SmoothArgs& a2, int threads, double* logD, double* rowmax, const double* w_t,
                         const int* dead, double* ws_t, double* cross_t, double* resid_t, hipStream_t s) {
    hipError_t e;
    const dim3 g1((unsigned)((a01.n + 255) / 256), (unsigned)a01.ntheta);
    if ((e = launch_pairs<MODEL, 0>(a01, threads, s)) != hipSuccess) return e;
    if (a01.nmax == 1 && a01.rmax == rowmax) {   // many chunks: the row maxima once per target
        hipLaunchKernelGGL(k_smooth_rowmax, g1, dim3(256), 0, s, a01.n, a01.ntheta, a01.nchunk, a01.pmax, rowmax);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if ((e = launch_pairs<MODEL, 1>(a01, threads, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_smooth_logd, g1, dim3(256), 0, s, a01.n, a01.ntheta, a01.nchunk, a01.rmax, a01.nmax, a01.part, logD);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = cross_t ? launch_pairs<MODEL, 3>(a2, threads, s) : launch_pairs<MODEL, 2>(a2, threads, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_smooth_finish, g1, dim3(256), 0, s, a2.n, a2.ntheta, a2.nchunk, a2.part, w_t, dead, ws_t);
    if ((e = hipGetLastError()) != hipSuccess || !cross_t) return e;
    hipLaunchKernelGGL((k_smooth_pair_moments<model_dim<MODEL>::value>), dim3((unsigned)a2.ntheta), dim3(PAIR_GROUP * SMOOTH_CH), 0, s, a2.n, a2.ntheta, a2.nchunk,
                       (const double*)a2.part, a2.x_own, w_t, dead, cross_t, resid_t);
    return hipGetLastError();
}

// what smc_smooth_quantiles adds to a backward pass: np levels p of state coordinate `component` -> q [T][n_theta][np]
struct SmoothQuantiles {
    int component, np;
    const double* p;
    double* q;
};

// smc_smooth, and with cross or resid2 smc_smooth_pairs: the same refusals, plan and launches; the pair moments add a block of
// their own (hist.d_pair: the chunk partials of PASS 3 and the results), so that a handle that never asks for them allocates and
// launches what it always did.  With sq (smc_smooth_quantiles) ONE launch more behind the pass, k_smooth_quantiles over the
// smoothed weights where the pass left them, and a block of its own again (hist.d_quant)
int smooth_run(smc_handle h, const char* name, double* ws, double* mean, double* var, double* cross, double* resid2,
               const SmoothQuantiles* sq = nullptr) {
    const std::string who = std::string(name) + ": ";
    if (!h) return fail(SMC_EINVAL, who + "NULL handle");
    if (!has_density(h->model))
        return fail(SMC_EINVAL, who + "SMC_MODEL_UCSV_RB has no transition density of its state rows (m and P are functions of the whole "
                                      "path); smooth a UCSV3D filter instead, or draw Rao-Blackwellised paths (smc_rb_sample_paths)");
    SmoothQArgs qa{};
    if (sq) {
        if (!sq->p || !sq->q) return fail(SMC_EINVAL, who + "NULL p or q");
        if (sq->np < 1 || sq->np > QMAX) return fail(SMC_EINVAL, who + "1 <= np <= 8");
        if (sq->component < 0 || sq->component >= h->d) return fail(SMC_EINVAL, who + "component outside [0, d)");
        for (int j = 0; j < sq->np; ++j) {
            if (!(sq->p[j] >= 0.0 && sq->p[j] <= 1.0)) return fail(SMC_EINVAL, who + "levels must lie in [0, 1]");
            qa.p64[j] = prob_to_u64(sq->p[j]);
        }
    }
    if (!h->hist.armed || h->hist.len < 1) return fail(SMC_ESTATE, who + "nothing is recorded (smc_history_begin, then smc_init / smc_step)");
    const FilterView& v = h->v;
    const int64_t T = h->hist.len, n = v.n;
    const size_t nw = cloud_words(h), nt = (size_t)v.ntheta, d = (size_t)h->d;
    const bool pairs = cross || resid2;
    if ((n + SMOOTH_CH - 1) / SMOOTH_CH > 65535) return fail(SMC_EINVAL, who + "more than 65535 chunks of particles (the backward pass is quadratic in n_x)");
    HIPCHK(hipSetDevice(h->device));
    std::vector<SmoothRow> rows;
    int rc = fetch_rows(h, h->model, name, "the transition scale", rows);
    if (rc) return rc;
    const SmoothPlan p = plan_of(h, T);
    // (the smoother's blocks: the old block first, unlike the walk's - DESIGN.md "Memory of a handle")
    if (h->hist.d_tmp.grow(p.bytes) != hipSuccess) return fail(SMC_ENOMEM, who + "hipMalloc of the scratch of the backward pass");
    const size_t mom_words = 2 * d * nt;
    if (T > h->hist.ws_cap) {
        h->hist.d_ws.reset();
        h->hist.ws_cap = 0;
        if (h->hist.d_ws.grow((size_t)h->hist.cap * (nw + mom_words) * 8) != hipSuccess) return fail(SMC_ENOMEM, who + "hipMalloc of the smoothed weights");
        h->hist.ws_cap = h->hist.cap;
    }
    // the pair moments: partials [1 + 2 d][nchunk][ntheta][n] | cross [cap - 1][d][d][ntheta] | resid2 [cap - 1][d][ntheta]
    const size_t cross_words = d * d * nt, resid_words = d * nt;
    double *d_pair = nullptr, *d_cross = nullptr, *d_resid = nullptr;
    if (pairs) {
        OffsetPlan o;
        const size_t steps = (size_t)h->hist.cap - 1;
        const size_t o_part = o.take((1 + 2 * d) * (size_t)p.nchunk * nw * 8), o_cross = o.take(steps * cross_words * 8), o_resid = o.take(steps * resid_words * 8);
        if (h->hist.d_pair.grow(o.bytes) != hipSuccess) return fail(SMC_ENOMEM, who + "hipMalloc of the chunk partials of the pair moments");
        char* pair = h->hist.d_pair.as<char>();
        d_pair = (double*)(pair + o_part); d_cross = (double*)(pair + o_cross); d_resid = (double*)(pair + o_resid);
    }
    // the quantiles: q [cap][ntheta][QMAX], and the kernel's LDS, all of it dynamic: the histograms and, for a cloud that is staged,
    // 16 bytes per particle (above 64 KiB the limit is raised)
    const size_t q_lds = SMOOTH_Q_FIXED_LDS + (n <= SMOOTH_Q_LDS_MAX ? (size_t)n * 16 : 0);
    if (sq) {
        static std::atomic<bool> raised[16];
        if (h->hist.d_quant.grow((size_t)h->hist.cap * nt * QMAX * 8) != hipSuccess) return fail(SMC_ENOMEM, who + "hipMalloc of the quantiles of the smoothed state");
        HIPCHK(raise_lds_limit(k_smooth_quantiles, q_lds, raised));
    }
    char* tmp = h->hist.d_tmp.as<char>();
    double *pmax = (double*)(tmp + p.o_pmax), *part = (double*)(tmp + p.o_part), *logD = (double*)(tmp + p.o_logD), *rowmax = (double*)(tmp + p.o_rmax), *momtmp = (double*)(tmp + p.o_mom);
    SmoothRow* d_rows = (SmoothRow*)(tmp + p.o_rows);
    int* dead = (int*)(tmp + p.o_dead);
    double *d_ws = h->hist.d_ws.as<double>(), *d_mom = d_ws + (size_t)h->hist.ws_cap * nw;
    hipStream_t s = h->stream;
    HIPCHK(hipEventRecord(h->ev0, s));
    HIPCHK(hipMemcpyAsync(d_rows, rows.data(), nt * sizeof(SmoothRow), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(dead, 0, nt * sizeof(int), s));
    hipLaunchKernelGGL(k_smooth_dead, dim3((unsigned)T, (unsigned)nt), dim3(256), 0, s, n, (int)nt, h->hist.d_w, dead);
    HIPCHK(hipGetLastError());
    // a lone small filter is cut into tiles of one wave, so that its few chunks still spread over the chip; the bits do not depend on it
    const int64_t wg256 = ((n + 255) / 256) * (int64_t)nt * p.nchunk;
    const int threads = wg256 >= 1024 ? 256 : 64;
    const dim3 g1((unsigned)((n + 255) / 256), (unsigned)nt);
    hipLaunchKernelGGL(k_smooth_finish, g1, dim3(256), 0, s, n, (int)nt, p.nchunk, (const double*)nullptr, h->hist.d_w + (size_t)(T - 1) * nw, dead,
                       d_ws + (size_t)(T - 1) * nw);
    HIPCHK(hipGetLastError());
    for (int64_t t = T - 2; t >= 0; --t) {
        const double *x_t = h->hist.d_x + (size_t)t * nw * d, *x_n = x_t + nw * d, *w_t = h->hist.d_w + (size_t)t * nw;
        double *ws_t = d_ws + (size_t)t * nw, *ws_n = ws_t + nw;
        const bool direct = p.nchunk <= SMOOTH_MAX_DIRECT;
        const SmoothArgs a01{n, (int)nt, p.nchunk, x_n, x_t, w_t, nullptr, pmax, direct ? pmax : rowmax, direct ? p.nchunk : 1, part, d_rows};
        const SmoothArgs a2{n, (int)nt, p.nchunk, x_t, x_n, ws_n, logD, pmax, nullptr, 0, pairs ? d_pair : part, d_rows};
        double *cross_t = pairs ? d_cross + (size_t)t * cross_words : nullptr, *resid_t = pairs ? d_resid + (size_t)t * resid_words : nullptr;
        HIPCHK(by_density_model(h->model, [&](auto Mt) {
            return backward_step<decltype(Mt)::value>(a01, a2, threads, logD, rowmax, w_t, dead, ws_t, cross_t, resid_t, s);
        }));
    }
    if (mean || var) {
        hipLaunchKernelGGL(k_smooth_moments, dim3((unsigned)T, (unsigned)nt), dim3(256), 0, s, n, (int)nt, p.nchunk, (int)d, h->hist.d_x, d_ws, dead,
                           momtmp, d_mom);
        HIPCHK(hipGetLastError());
    }
    if (sq) {
        qa.n = n; qa.ntheta = (int)nt; qa.d = (int)d; qa.component = sq->component; qa.np = sq->np;
        qa.x = h->hist.d_x; qa.ws = d_ws; qa.out = h->hist.d_quant.as<double>();
        hipLaunchKernelGGL(k_smooth_quantiles, dim3((unsigned)T, (unsigned)nt), dim3(SMOOTH_Q_THREADS), q_lds, s, qa);
        HIPCHK(hipGetLastError());
    }
    if ((rc = finish_elapsed(h))) return rc;
    if (sq) HIPCHK(hipMemcpy(sq->q, h->hist.d_quant.as<double>(), (size_t)T * nt * (size_t)sq->np * 8, hipMemcpyDeviceToHost));
    if (ws) HIPCHK(hipMemcpy(ws, d_ws, (size_t)T * nw * 8, hipMemcpyDeviceToHost));
    if (mean || var) {
        std::vector<double> mv((size_t)T * mom_words);
        HIPCHK(hipMemcpy(mv.data(), d_mom, mv.size() * 8, hipMemcpyDeviceToHost));
        for (int64_t t = 0; t < T; ++t) {
            if (mean) memcpy(mean + (size_t)t * d * nt, mv.data() + (size_t)t * mom_words, d * nt * 8);
            if (var) memcpy(var + (size_t)t * d * nt, mv.data() + (size_t)t * mom_words + d * nt, d * nt * 8);
        }
    }
    if (cross && T > 1) HIPCHK(hipMemcpy(cross, d_cross, (size_t)(T - 1) * cross_words * 8, hipMemcpyDeviceToHost));
    if (resid2 && T > 1) HIPCHK(hipMemcpy(resid2, d_resid, (size_t)(T - 1) * resid_words * 8, hipMemcpyDeviceToHost));
    return SMC_OK;
}
}  // namespace

extern "C" int smc_smooth(smc_handle h, double* ws, double* mean, double* var) { return smooth_run(h, "smc_smooth", ws, mean, var, nullptr, nullptr); }

extern "C" int smc_smooth_pairs(smc_handle h, double* ws, double* mean, double* var, double* cross, double* resid2) {
    return smooth_run(h, "smc_smooth_pairs", ws, mean, var, cross, resid2);
}

extern "C" int smc_smooth_quantiles(smc_handle h, double* ws, double* mean, double* var, double* cross, double* resid2, int component,
                                    const double* p, int np, double* q) {
    const SmoothQuantiles sq{component, np, p, q};
    return smooth_run(h, "smc_smooth_quantiles", ws, mean, var, cross, resid2, &sq);
}

// the constants of the quantiles of the smoothed state, and the bytes of the handle's quantile block (0: it never asked for them)
extern "C" int smc_smooth_quantiles_info(smc_handle h, int64_t* scratch_bytes, int32_t* q_bits, int64_t* lds_max) {
    if (scratch_bytes) *scratch_bytes = h ? (int64_t)h->hist.d_quant.bytes() : 0;
    if (q_bits) *q_bits = SMOOTH_Q_BITS;
    if (lds_max) *lds_max = SMOOTH_Q_LDS_MAX;
    return SMC_OK;
}

// ---- backward simulation ---------------------------------------------------------------------------------------------------
namespace {
template <int MODEL>
hipError_t path_step(const PathArgs& a, int threads, double* rowmax, hipStream_t s) {
    hipError_t e;
    const dim3 grid((unsigned)((a.M + threads - 1) / threads), (unsigned)a.ntheta, (unsigned)a.nchunk), g1((unsigned)((a.M + 255) / 256), (unsigned)a.ntheta);
    hipLaunchKernelGGL((k_path_pairs<MODEL, 0>), grid, dim3(threads), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (a.nmax == 1 && a.rmax == rowmax) {   // many chunks: the maximum once per path, as the smoother takes it once per target
        hipLaunchKernelGGL(k_smooth_rowmax, g1, dim3(256), 0, s, a.M, a.ntheta, a.nchunk, a.pmax, rowmax);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL((k_path_pairs<MODEL, 1>), grid, dim3(threads), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (a.M * (int64_t)a.ntheta < PATH_WAVE_SELECT)   // few paths: one wave per path (four per workgroup)
        hipLaunchKernelGGL((k_path_select_wave<MODEL>), dim3((unsigned)((a.M + 3) / 4), (unsigned)a.ntheta), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((k_path_select<MODEL>), dim3((unsigned)((a.M + 63) / 64), (unsigned)a.ntheta), dim3(64), 0, s, a);
    return hipGetLastError();
}

// One backward walk over the record, M paths per filter: what its caller sets ...
struct Walk {
    const char *who, *what;   // the entry point, at the head of every message, and its wording for a row smooth_row refuses
    int row_model;            // the family whose constants smooth_row derives from the rows
    size_t cur_rows;          // state rows a path carries from step to step
    size_t step_words;        // words per path and step over everything the block holds (the check that its sizes fit size_t)
    const double* y;          // the observations the recorded steps saw, T of them (PathArgs::y, checked against the record), or nullptr
    int64_t T;
    // ... what the tail of its plan adds: the observations on the device (with y) and the states of the paths, xs_rows per step (0: none)
    size_t o_y, o_xs, xs_rows;
    // ... and what the walk leaves in hist.d_path for what follows it (offsets in bytes)
    size_t o_counts, o_idx;
};
// The refusals the two entry points share, the plan of the block (the common prefix cur | pmax | psum | rmax | rows | dead | counts |
// idx, then tail(plan, T, pw): the caller's arrays), the block itself, the uploads, the dead scan and the loop over the steps, all on
// the handle's stream behind ev0.  The caller adds what follows and closes the timed region (finish_elapsed).
template <class Tail>
int backward_walk(smc_handle h, Walk& k, int64_t M, uint64_t path_seed, const int32_t* counts, Tail&& tail) {
    const std::string who = std::string(k.who) + ": ";
    if (M < 1 || M > ((int64_t)1 << 30)) return fail(SMC_EINVAL, who + "M must be in [1, 2^30]");
    if (!h->hist.armed || h->hist.len < 1) return fail(SMC_ESTATE, who + "nothing is recorded (smc_history_begin, then smc_init / smc_step)");
    const FilterView& v = h->v;
    const int64_t T = h->hist.len, n = v.n;
    if (k.y) {
        if (k.T != T) return fail(SMC_EINVAL, who + "T is not the number of recorded steps (smc_history_len)");
        for (int64_t t = 0; t < T; ++t)
            if (!(k.y[t] - k.y[t] == 0.0)) return fail(SMC_EINVAL, who + "y[" + std::to_string(t) + "] is not finite");
    }
    const size_t nw = cloud_words(h), nt = (size_t)v.ntheta, d = (size_t)h->d, pw = nt * (size_t)M;
    if (n > PATH_MAX_N) return fail(SMC_EINVAL, who + "more than 2^20 particles per filter (the integer weights of a step would not fit their sum)");
    std::vector<int32_t> cnt(nt, (int32_t)M);
    for (size_t m = 0; counts && m < nt; ++m) {
        if (counts[m] < 0 || counts[m] > M) return fail(SMC_EINVAL, who + "counts[" + std::to_string(m) + "] is outside [0, M]");
        cnt[m] = counts[m];
    }
    HIPCHK(hipSetDevice(h->device));
    std::vector<SmoothRow> rows;
    const int rc = fetch_rows(h, k.row_model, k.who, k.what, rows);
    if (rc) return rc;
    const int nchunk = (int)((n + SMOOTH_CH - 1) / SMOOTH_CH);
    if (pw > ((size_t)1 << 56) / ((size_t)T * k.step_words) || pw > ((size_t)1 << 56) / (size_t)nchunk)
        return fail(SMC_ENOMEM, who + "paths of that many bytes cannot be allocated");
    OffsetPlan p;
    const size_t o_cur = p.take(k.cur_rows * pw * 8), o_pmax = p.take((size_t)nchunk * pw * 8), o_psum = p.take((size_t)nchunk * pw * 8),
                 o_rmax = p.take(pw * 8), o_rows = p.take(nt * sizeof(SmoothRow)), o_dead = p.take(nt * sizeof(int));
    k.o_counts = p.take(nt * sizeof(int32_t));
    k.o_idx = p.take((size_t)T * pw * 4);
    tail(p, (size_t)T, pw);
    // (the new block first: a failed allocation leaves the handle as it was)
    if (h->hist.d_path.grow_keep(p.bytes) != hipSuccess) return fail(SMC_ENOMEM, who + "hipMalloc of the paths and the scratch of the backward walk");
    char* base = h->hist.d_path.as<char>();
    double *cur = (double*)(base + o_cur), *pmax = (double*)(base + o_pmax), *rowmax = (double*)(base + o_rmax);
    uint64_t* psum = (uint64_t*)(base + o_psum);
    SmoothRow* d_rows = (SmoothRow*)(base + o_rows);
    int* dead = (int*)(base + o_dead);
    int32_t *d_counts = (int32_t*)(base + k.o_counts), *d_idx = (int32_t*)(base + k.o_idx);
    double* d_xs = k.xs_rows ? (double*)(base + k.o_xs) : nullptr;
    hipStream_t s = h->stream;
    HIPCHK(hipEventRecord(h->ev0, s));
    HIPCHK(hipMemcpyAsync(d_rows, rows.data(), nt * sizeof(SmoothRow), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_counts, cnt.data(), nt * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (k.y) HIPCHK(hipMemcpyAsync(base + k.o_y, k.y, (size_t)T * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(dead, 0, nt * sizeof(int), s));
    hipLaunchKernelGGL(k_smooth_dead, dim3((unsigned)T, (unsigned)nt), dim3(256), 0, s, n, (int)nt, h->hist.d_w, dead);
    HIPCHK(hipGetLastError());
    // the smoother's rule: a launch of few workgroups is cut into tiles of one wave; the bits do not depend on it
    const int64_t wg256 = ((M + 255) / 256) * (int64_t)nt * nchunk;
    const int threads = wg256 >= 1024 ? 256 : 64;
    const bool direct = nchunk <= SMOOTH_MAX_DIRECT;
    for (int64_t t = T - 1; t >= 0; --t) {
        PathArgs a{};
        a.n = n; a.M = M; a.ntheta = (int)nt; a.nchunk = nchunk;
        a.last = t == T - 1; a.t = (uint32_t)t; a.seed = path_seed;
        if (k.y) a.y = k.y[t];
        a.x_t = h->hist.d_x + (size_t)t * nw * d; a.w_t = h->hist.d_w + (size_t)t * nw;
        a.cur = cur; a.pmax = pmax; a.rmax = direct ? pmax : rowmax; a.nmax = direct ? nchunk : 1; a.psum = psum;
        a.rows = d_rows; a.dead = dead; a.counts = d_counts; a.stream = h->d_stream;
        a.idx_n = d_idx + (size_t)(t + 1 < T ? t + 1 : t) * pw; a.idx_t = d_idx + (size_t)t * pw;
        a.xs_t = d_xs ? d_xs + (size_t)t * k.xs_rows * pw : nullptr;
        HIPCHK(by_model(h->model, [&](auto Mt) { return path_step<decltype(Mt)::value>(a, threads, rowmax, s); }));
    }
    return SMC_OK;
}
}  // namespace

extern "C" int smc_sample_paths(smc_handle h, int64_t M, uint64_t path_seed, const int32_t* counts, int32_t* idx, double* xs) {
    if (!h) return fail(SMC_EINVAL, "smc_sample_paths: NULL handle");
    if (!has_density(h->model))
        return fail(SMC_EINVAL, "smc_sample_paths: SMC_MODEL_UCSV_RB has no transition density of its state rows (m and P are functions of the "
                                "whole path); draw the paths of a UCSV3D filter instead, or call smc_rb_sample_paths");
    const size_t d = (size_t)h->d;
    Walk k{"smc_sample_paths", "the transition scale", h->model, d, d + 1, nullptr, 0};
    size_t T = 0, pw = 0;
    int rc = backward_walk(h, k, M, path_seed, counts, [&](OffsetPlan& p, size_t T_, size_t pw_) {
        T = T_; pw = pw_;
        k.xs_rows = xs ? d : 0;
        k.o_xs = p.take(xs ? T * d * pw * 8 : 0);
    });
    h->hist.walk_M = 0;   // (a walk that fails leaves nothing to gather through)
    if (rc || (rc = finish_elapsed(h))) return rc;
    h->hist.walk_M = M; h->hist.walk_T = (int64_t)T; h->hist.walk_idx = k.o_idx;   // smc_reference_from_paths
    const char* base = h->hist.d_path.as<char>();
    if (idx) HIPCHK(hipMemcpy(idx, base + k.o_idx, T * pw * 4, hipMemcpyDeviceToHost));
    if (xs) HIPCHK(hipMemcpy(xs, base + k.o_xs, T * d * pw * 8, hipMemcpyDeviceToHost));
    return SMC_OK;
}

// ---- Rao-Blackwellised backward simulation (MODEL_UCSV_RB) ---------------------------------------------------------------------
extern "C" int smc_rb_sample_paths(smc_handle h, const double* y, int64_t T, int64_t M, uint64_t path_seed, const int32_t* counts, int32_t* idx,
                                   double* vol, double* tmean, double* tvar, double* tdraw, double* out) {
    if (!h) return fail(SMC_EINVAL, "smc_rb_sample_paths: NULL handle");
    if (h->model != MODEL_UCSV_RB)
        return fail(SMC_EINVAL, "smc_rb_sample_paths: the handle is not SMC_MODEL_UCSV_RB (the other families have a transition density: smc_sample_paths)");
    if (!y) return fail(SMC_EINVAL, "smc_rb_sample_paths: NULL y");
    if (T > 0 && series_has_gap(h, y, T))
        return fail(SMC_EINVAL, "smc_rb_sample_paths: y holds a NaN and the handle reads NaN as missing (SMC_FLAG_NAN_MISSING): the Kalman / RTS pass "
                                "along a path has no rule for a gap yet");
    // (the two gammas are UCSV3D's: nh1, nh2; a path carries (lse, lsn, mu, tau) and records (lse, lsn))
    Walk k{"smc_rb_sample_paths", "a gamma", MODEL_UCSV3D, 4, 8, y, T};
    h->hist.walk_M = 0;   // (the block is laid out anew)
    const size_t nt = (size_t)h->v.ntheta;
    int mchunk = 0;   // chunks of paths (the summary)
    size_t pw = 0, o_tmean = 0, o_tvar = 0, o_tdraw = 0, o_stmp = 0, o_out = 0;
    int rc = backward_walk(h, k, M, path_seed, counts, [&](OffsetPlan& p, size_t, size_t pw_) {
        pw = pw_;
        mchunk = (int)((M + SMOOTH_CH - 1) / SMOOTH_CH);
        k.o_y = p.take((size_t)T * 8);
        k.xs_rows = 2;
        k.o_xs = p.take((size_t)T * 2 * pw * 8);
        o_tmean = p.take((size_t)T * pw * 8);
        o_tvar = p.take((size_t)T * pw * 8);
        o_tdraw = p.take(tdraw ? (size_t)T * pw * 8 : 0);
        o_stmp = p.take((size_t)T * nt * (size_t)mchunk * 8);
        o_out = p.take((size_t)T * nt * 8 * 8);
    });
    if (rc) return rc;
    char* base = h->hist.d_path.as<char>();
    const double* d_y = (const double*)(base + k.o_y);
    const int32_t *d_counts = (const int32_t*)(base + k.o_counts), *d_idx = (const int32_t*)(base + k.o_idx);
    double *d_vol = (double*)(base + k.o_xs), *d_tmean = (double*)(base + o_tmean), *d_tvar = (double*)(base + o_tvar);
    double *d_tdraw = tdraw ? (double*)(base + o_tdraw) : nullptr, *d_stmp = (double*)(base + o_stmp), *d_out = (double*)(base + o_out);
    hipStream_t s = h->stream;
    RbTrendArgs ta{T, M, (int)nt, path_seed, h->d_params, h->d_stream, d_y, d_idx, d_vol, d_tmean, d_tvar, d_tdraw};
    hipLaunchKernelGGL(k_rb_trend, dim3((unsigned)((M + 63) / 64), (unsigned)nt), dim3(64), 0, s, ta);
    HIPCHK(hipGetLastError());
    if (out) {
        hipLaunchKernelGGL(k_rb_summary, dim3((unsigned)T, (unsigned)nt), dim3(256), 0, s, M, (int)nt, mchunk, d_idx, d_counts, d_tmean, d_tvar, d_vol,
                           d_stmp, d_out);
        HIPCHK(hipGetLastError());
    }
    if ((rc = finish_elapsed(h))) return rc;
    if (idx) HIPCHK(hipMemcpy(idx, d_idx, (size_t)T * pw * 4, hipMemcpyDeviceToHost));
    if (vol) HIPCHK(hipMemcpy(vol, d_vol, (size_t)T * 2 * pw * 8, hipMemcpyDeviceToHost));
    if (tmean) HIPCHK(hipMemcpy(tmean, d_tmean, (size_t)T * pw * 8, hipMemcpyDeviceToHost));
    if (tvar) HIPCHK(hipMemcpy(tvar, d_tvar, (size_t)T * pw * 8, hipMemcpyDeviceToHost));
    if (tdraw) HIPCHK(hipMemcpy(tdraw, d_tdraw, (size_t)T * pw * 8, hipMemcpyDeviceToHost));
    if (out) HIPCHK(hipMemcpy(out, d_out, (size_t)T * nt * 8 * 8, hipMemcpyDeviceToHost));
    return SMC_OK;
}

// ---- ancestor sampling: the sweep of a conditional handle without the walk (smc_spec.h "ancestor sampling") ------------
int ancestor_sweep_enqueue(smc_handle h, uint64_t path_seed, const int32_t** d_J, const int32_t** d_idx, const int** d_dead) {
    const FilterView& v = h->v;
    const int64_t T = h->hist.len, n = v.n;
    const size_t nt = (size_t)v.ntheta;
    HIPCHK(hipSetDevice(h->device));
    std::vector<SmoothRow> rows;
    const int rc = fetch_rows(h, h->model, "smc_ancestor_sweep", "the transition scale", rows);   // (waits for the steps)
    if (rc) return rc;
    OffsetPlan p;
    const size_t o_J = p.take((size_t)T * nt * 4), o_idx = p.take((size_t)T * nt * 4), o_last = p.take(nt * 4), o_dead = p.take(nt * sizeof(int)),
                 o_rows = p.take(nt * sizeof(SmoothRow));
    // (the new block first: a failed allocation leaves the handle as it was; the stream is idle after fetch_rows)
    if (h->cond.d_sweep.grow_keep(p.bytes) != hipSuccess) return fail(SMC_ENOMEM, "smc_ancestor_sweep: hipMalloc of the indices of the sweep");
    char* base = h->cond.d_sweep.as<char>();
    AncArgs a{};
    a.n = n; a.T = T; a.ntheta = (int)nt; a.d = h->d;
    a.seed = v.seed; a.path_seed = path_seed;
    a.hx = h->hist.d_x; a.hw = h->hist.d_w; a.ha = h->hist.d_a;
    a.xref = h->cond.d_xref.as<double>();
    a.rows = (const SmoothRow*)(base + o_rows); a.stream = h->d_stream;
    a.J = (int32_t*)(base + o_J); a.idx = (int32_t*)(base + o_idx); a.last = (int32_t*)(base + o_last); a.dead = (int*)(base + o_dead);
    hipStream_t s = h->stream;
    HIPCHK(hipMemcpyAsync(base + o_rows, rows.data(), nt * sizeof(SmoothRow), hipMemcpyHostToDevice, s));
    // ONE launch for the T - 1 ancestor draws and the last pick: a workgroup per (step, filter); one wave when the cloud is small
    const int threads = n <= ANC_WAVE_N ? 64 : 256;
    HIPCHK(by_density_model(h->model, [&](auto Mt) {
        hipLaunchKernelGGL((k_cond_ancestors<decltype(Mt)::value>), dim3((unsigned)T, (unsigned)nt), dim3(threads), 0, s, a);
        return hipGetLastError();
    }));
    hipLaunchKernelGGL(k_cond_trace, dim3((unsigned)((nt + 63) / 64)), dim3(64), 0, s, a);
    HIPCHK(hipGetLastError());
    *d_J = a.J; *d_idx = a.idx; *d_dead = a.dead;
    return SMC_OK;
}
