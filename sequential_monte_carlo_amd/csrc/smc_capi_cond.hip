// smc_capi_cond.hip -- the reference trajectory of a conditional handle (SMC_FLAG_CONDITIONAL; include/smc_hip.h "the conditional
// particle filter"): smc_set_reference, smc_get_reference and smc_reference_from_paths, the device gather of one backward-simulated
// path out of the record into the reference's own buffer.  The conditional step itself: smc_kernels.h (COND), launched by do_init /
// do_step (smc_capi.hip).  Specification: smc_spec.h "the conditional particle filter".  Also smc_ancestor_sweep, the sweep of a
// handle with SMC_FLAG_ANCESTOR_SAMPLING (smc_spec.h "ancestor sampling"): its refusals and results; its launches live with the record.
#include "smc_host.h"

#include <vector>

using namespace smc;

namespace {
// xref[t][c][th] = x_t[c][th][idx[t][th][p]] for the filters whose path p is complete (idx[0][th][p] >= 0); the others keep their row.
// One thread per (t, th); grid (ceil(ntheta / 128), min(T, 65535))
__global__ __launch_bounds__(128) void k_reference_gather(int64_t T, int64_t n, int ntheta, int d, int64_t M, int64_t p, const double* __restrict__ hx /*[T][d][ntheta][n]*/,
                                                          const int32_t* __restrict__ idx /*[T][ntheta][M]*/, double* __restrict__ xref /*[T][d][ntheta]*/) {
    const int th = (int)(blockIdx.x * 128u + threadIdx.x);
    if (th >= ntheta) return;
    const size_t pw = (size_t)ntheta * (size_t)M, at = (size_t)th * (size_t)M + (size_t)p;
    if (idx[at] < 0) return;   // a dead path: -1 at step 0 (and then at every step)
    for (size_t t = blockIdx.y; t < (size_t)T; t += gridDim.y) {
        const int32_t i = idx[t * pw + at];
        if (i < 0 || (int64_t)i >= n) continue;   // (never on a complete path: the walk's indices are particles)
        for (int c = 0; c < d; ++c)
            xref[(t * (size_t)d + (size_t)c) * (size_t)ntheta + (size_t)th] = hx[((t * (size_t)d + (size_t)c) * (size_t)ntheta + (size_t)th) * (size_t)n + (size_t)i];
    }
}

int need_conditional(smc_handle h, const char* who) {
    if (!h) return fail(SMC_EINVAL, std::string(who) + ": NULL handle");
    if (!conditional(h)) return fail(SMC_ESTATE, std::string(who) + ": the handle was not created with SMC_FLAG_CONDITIONAL");
    return SMC_OK;
}
}  // namespace

extern "C" int smc_set_reference(smc_handle h, const double* xref, int64_t T) {
    int rc = need_conditional(h, "smc_set_reference");
    if (rc) return rc;
    if (!xref || T < 1) return fail(SMC_EINVAL, "smc_set_reference: NULL reference or T < 1");
    const size_t row = (size_t)h->d * (size_t)h->v.ntheta;
    if ((size_t)T > ((size_t)1 << 56) / row) return fail(SMC_ENOMEM, "smc_set_reference: a reference of that many bytes cannot be allocated");
    const size_t words = (size_t)T * row;
    for (size_t i = 0; i < words; ++i)
        if (!finite_d(xref[i])) return fail(SMC_EINVAL, "smc_set_reference: entry " + std::to_string(i) + " of the reference is not finite");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    // (the new block first: a failed allocation leaves the handle as it was)
    if (h->cond.d_xref.grow_keep(words * 8) != hipSuccess) return fail(SMC_ENOMEM, "smc_set_reference: hipMalloc of the reference");
    h->cond.T = T;
    HIPCHK(hipMemcpy(h->cond.d_xref.as<double>(), xref, words * 8, hipMemcpyHostToDevice));
    return SMC_OK;
}

extern "C" int smc_get_reference(smc_handle h, double* xref, int64_t* T) {
    int rc = need_conditional(h, "smc_get_reference");
    if (rc) return rc;
    if (!h->cond.d_xref) return fail(SMC_ESTATE, "smc_get_reference: the handle has no reference (smc_set_reference)");
    if (T) *T = h->cond.T;
    if (!xref) return SMC_OK;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(xref, h->cond.d_xref.as<double>(), (size_t)h->cond.T * (size_t)h->d * (size_t)h->v.ntheta * 8, hipMemcpyDeviceToHost));
    return SMC_OK;
}

extern "C" int smc_reference_from_paths(smc_handle h, int64_t p, int64_t* kept) {
    int rc = need_conditional(h, "smc_reference_from_paths");
    if (rc) return rc;
    if (!h->hist.armed || h->hist.walk_M < 1 || !h->hist.d_path || h->hist.walk_T != h->hist.len)
        return fail(SMC_ESTATE, "smc_reference_from_paths: no smc_sample_paths walk over the handle's current record");
    const int64_t M = h->hist.walk_M, T = h->hist.walk_T;
    if (p < 0 || p >= M) return fail(SMC_EINVAL, "smc_reference_from_paths: p is not a path of the last walk");
    const size_t nt = (size_t)h->v.ntheta, d = (size_t)h->d;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int32_t* d_idx = (const int32_t*)(h->hist.d_path.as<char>() + h->hist.walk_idx);
    // the filters whose path is dead keep their reference: they are counted first, because a reference of another length (or none)
    // has nothing for them to keep
    std::vector<int32_t> first(nt);
    HIPCHK(hipMemcpy2D(first.data(), 4, d_idx + p, (size_t)M * 4, 4, nt, hipMemcpyDeviceToHost));
    int64_t nkept = 0;
    for (size_t m = 0; m < nt; ++m) nkept += first[m] < 0;
    if (nkept && (!h->cond.d_xref || h->cond.T != T))
        return fail(SMC_ESTATE, "smc_reference_from_paths: path p of " + std::to_string(nkept) + " filter(s) is dead and the handle has no reference of " +
                                    std::to_string(T) + " steps for them to keep");
    if (h->cond.d_xref.grow_keep((size_t)T * d * nt * 8) != hipSuccess) return fail(SMC_ENOMEM, "smc_reference_from_paths: hipMalloc of the reference");
    h->cond.T = T;
    hipLaunchKernelGGL(k_reference_gather, dim3((unsigned)((nt + 127) / 128), (unsigned)(T < 65535 ? T : 65535)), dim3(128), 0, h->stream, T, (int64_t)h->v.n, (int)nt, (int)d, M, p,
                       (const double*)h->hist.d_x, d_idx, h->cond.d_xref.as<double>());
    HIPCHK(hipGetLastError());
    if (kept) *kept = nkept;
    return SMC_OK;   // no wait: the next sweep's launches are ordered behind the gather on the handle's stream
}

// ---- ancestor sampling (include/smc_hip.h "ancestor sampling"): the refusals and the results; the launches: smc_capi_smooth.hip ------
extern "C" int smc_ancestor_sweep(smc_handle h, uint64_t path_seed, int32_t* J, int32_t* idx, int64_t* kept) {
    if (!h) return fail(SMC_EINVAL, "smc_ancestor_sweep: NULL handle");
    if (!ancestor_sampling(h)) return fail(SMC_ESTATE, "smc_ancestor_sweep: the handle was not created with SMC_FLAG_ANCESTOR_SAMPLING");
    if (!h->cond.d_xref) return fail(SMC_ESTATE, "smc_ancestor_sweep: the handle has no reference (smc_set_reference)");
    if (!h->hist.armed || !h->hist.d_a || h->hist.len < 1)
        return fail(SMC_ESTATE, "smc_ancestor_sweep: nothing is recorded (smc_history_begin, then smc_init / smc_step)");
    if (h->hist.len != h->cond.T)
        return fail(SMC_ESTATE, "smc_ancestor_sweep: " + std::to_string(h->hist.len) + " steps are recorded and the reference has " + std::to_string(h->cond.T) +
                                    " (the sweep wants the whole run over the reference)");
    const int32_t *d_J = nullptr, *d_idx = nullptr;
    const int* d_dead = nullptr;
    const int rc = ancestor_sweep_enqueue(h, path_seed, &d_J, &d_idx, &d_dead);
    if (rc || (!J && !idx && !kept)) return rc;   // nothing asked for: no wait, the next sweep's launches are ordered behind these
    const size_t nt = (size_t)h->v.ntheta, words = (size_t)h->hist.len * nt;
    HIPCHK(hipStreamSynchronize(h->stream));
    if (J) HIPCHK(hipMemcpy(J, d_J, words * 4, hipMemcpyDeviceToHost));
    if (idx) HIPCHK(hipMemcpy(idx, d_idx, words * 4, hipMemcpyDeviceToHost));
    if (kept) {
        std::vector<int> dead(nt);
        HIPCHK(hipMemcpy(dead.data(), d_dead, nt * sizeof(int), hipMemcpyDeviceToHost));
        *kept = 0;
        for (size_t m = 0; m < nt; ++m) *kept += dead[m] != 0;
    }
    return SMC_OK;
}
