// smc_capi_slots.hip -- the state of the filters as data: read-back (smc_get_state, smc_get_weights_raw) and the exchange of
// whole filters between slots, handles and ranks (smc_permute, smc_copy_from, smc_pack_slots / smc_unpack_slots); kernels in
// smc_slot_kernels.h.
#include "smc_host.h"
#include "smc_slot_kernels.h"

#include <cstring>

using namespace smc;

hipError_t copy_slots(const FilterView& dst, int dcur, const FilterView& src, int scur, int d, const unsigned char* mask, hipStream_t s) {
    hipLaunchKernelGGL(k_copy_slots, dim3((unsigned)((dst.npad + 255) / 256), dst.ntheta), dim3(256), 0, s, dst, dcur, src, scur, d, mask);
    return hipGetLastError();
}

int ensure_wdense(smc_handle h) {   // [ntheta][n] dense weights, with room for the moments [2][d][ntheta] (smc_get_moments) from the start
    HIPCHK(h->d_wdense.grow(((size_t)h->v.ntheta * (size_t)h->v.n + 2 * (size_t)h->d * (size_t)h->v.ntheta) * 8));
    return SMC_OK;
}

hipError_t enqueue_dense_weights(smc_filter_s* h, double* w) {
    const FilterView& v = h->v;
    hipLaunchKernelGGL(k_dense_weights, dim3((unsigned)((v.n + 255) / 256), v.ntheta), dim3(256), 0, h->stream, v, h->cur, w);
    return hipGetLastError();
}

extern "C" int smc_get_state(smc_handle h, double* x, double* w, int32_t* anc) {
    if (!h) return fail(SMC_EINVAL, "smc_get_state: NULL handle");
    if (!h->inited) return fail(SMC_ESTATE, "smc_get_state: filter not initialised");
    HIPCHK(hipSetDevice(h->device));
    const FilterView& v = h->v;
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t rows = (size_t)h->d * v.ntheta;
    if (x)
        HIPCHK(hipMemcpy2D(x, (size_t)v.n * 8, v.x[h->cur], (size_t)v.npad * 8, (size_t)v.n * 8, rows,
                           hipMemcpyDeviceToHost));
    if (anc) {
        if (!v.anc) return fail(SMC_ESTATE, "smc_get_state: handle created without SMC_FLAG_ANCESTORS");
        HIPCHK(hipMemcpy2D(anc, (size_t)v.n * 4, v.anc, (size_t)v.npad * 4, (size_t)v.n * 4, (size_t)v.ntheta,
                           hipMemcpyDeviceToHost));
    }
    if (w) {
        int rc = emit_if_needed(h);
        if (rc) return rc;
        if ((rc = ensure_wdense(h))) return rc;
        HIPCHK(enqueue_dense_weights(h, h->d_wdense.as<double>()));
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipMemcpy(w, h->d_wdense.as<double>(), (size_t)v.ntheta * v.n * 8, hipMemcpyDeviceToHost));
    }
    return SMC_OK;
}

extern "C" int smc_permute(smc_handle h, const int32_t* a) {
    if (!h || !a) return fail(SMC_EINVAL, "smc_permute: NULL argument");
    if (!h->inited) return fail(SMC_ESTATE, "smc_permute: filter not initialised");
    if (history_armed(h)) return history_refuse("smc_permute");
    for (int m = 0; m < h->v.ntheta; ++m)
        if (a[m] < 0 || a[m] >= h->v.ntheta) return fail(SMC_EINVAL, "smc_permute: index out of range");
    h->win.k = 0;   // (behind every refusal: a refused call leaves the handle as it was)
    HIPCHK(hipSetDevice(h->device));
    int rc = emit_if_needed(h);
    if (rc) return rc;
    const FilterView& v = h->v;
    // The call returns without waiting for the device (whatever follows on this handle is ordered behind on its stream; the host
    // goes on with the random-walk covariance meanwhile): the indices travel from a pinned copy the handle owns.
    if (!h->h_perm) HIPCHK(h->h_perm.grow((size_t)v.ntheta * 4));
    else HIPCHK(hipStreamSynchronize(h->stream));   // (a previous permutation's copy out of the same buffer has completed)
    memcpy(h->h_perm.as<int32_t>(), a, (size_t)v.ntheta * 4);
    HIPCHK(hipMemcpyAsync(h->d_perm, h->h_perm.as<int32_t>(), (size_t)v.ntheta * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_logZ_tmp, v.logZ, (size_t)v.ntheta * 8, hipMemcpyDeviceToDevice, h->stream));
    hipLaunchKernelGGL(k_permute, dim3((unsigned)((v.npad + 255) / 256), v.ntheta), dim3(256), 0, h->stream, v, h->cur, h->d,
                       h->d_perm, h->d_logZ_tmp);
    HIPCHK(hipGetLastError());
    hot_invalidate(h);   // slots moved on the device
    h->cur ^= 1;
    // last_* (g, D, logmu, ess) describe slot-local weights: recompute them for the new layout
    HIPCHK(hipMemcpyAsync(h->d_logZ_tmp, v.logZ, (size_t)v.ntheta * 8, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(do_finalize(h, 0, h->t - 1));
    HIPCHK(hipMemcpyAsync(v.logZ, h->d_logZ_tmp, (size_t)v.ntheta * 8, hipMemcpyDeviceToDevice, h->stream));
    return SMC_OK;
}

extern "C" int smc_copy_from(smc_handle dst, smc_handle src, const uint8_t* mask) {
    if (!dst || !src || !mask) return fail(SMC_EINVAL, "smc_copy_from: NULL argument");
    if (dst == src) return fail(SMC_EINVAL, "smc_copy_from: dst and src are the same handle");
    if (!dst->inited || !src->inited) return fail(SMC_ESTATE, "smc_copy_from: filter not initialised");
    if (history_armed(dst)) return history_refuse("smc_copy_from");
    const FilterView &a = dst->v, &b = src->v;
    if (dst->model != src->model || a.n != b.n || a.seg != b.seg || a.ntheta != b.ntheta || dst->device != src->device)
        return fail(SMC_EINVAL, "smc_copy_from: handles differ in model, geometry or device");
    dst->win.k = 0;   // (behind every refusal)
    HIPCHK(hipSetDevice(dst->device));
    int rc = emit_if_needed(dst);
    if (rc) return rc;
    rc = emit_if_needed(src);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(src->stream));
    unsigned char* d_mask = reinterpret_cast<unsigned char*>(dst->d_perm);   // n_theta bytes fit in n_theta int32
    HIPCHK(hipMemcpyAsync(d_mask, mask, (size_t)a.ntheta, hipMemcpyHostToDevice, dst->stream));
    HIPCHK(copy_slots(a, dst->cur, b, src->cur, dst->d, d_mask, dst->stream));
    hot_invalidate(dst);
    HIPCHK(hipStreamSynchronize(dst->stream));
    dst->t = src->t;   // the accepted filters have seen the same observations
    return SMC_OK;
}

extern "C" int smc_slot_bytes(smc_handle h, int64_t* bytes) {
    if (!h || !bytes) return fail(SMC_EINVAL, "smc_slot_bytes: NULL argument");
    *bytes = slot_words(h->d, h->v.npad, h->v.nseg) * 8;
    return SMC_OK;
}

static int pack_unpack(smc_handle h, const int32_t* idx, int64_t k, void* buf, bool pack) {
    if (!h || k < 0 || (k > 0 && (!idx || !buf))) return fail(SMC_EINVAL, "smc_pack/unpack_slots: bad argument");
    if (!h->inited) return fail(SMC_ESTATE, "smc_pack/unpack_slots: filter not initialised");
    if (!pack && history_armed(h)) return history_refuse("smc_unpack_slots");
    for (int64_t i = 0; i < k; ++i)
        if (idx[i] < 0 || idx[i] >= h->v.ntheta) return fail(SMC_EINVAL, "smc_pack/unpack_slots: index out of range");
    if (!pack) h->win.k = 0;   // (behind every refusal: a refused call leaves the pending window and the by-value copies alone)
    if (k == 0) return SMC_OK;
    if (!pack) hot_invalidate(h);   // slots written on the device (the exchange of smc_comm.hip ends here too)
    HIPCHK(hipSetDevice(h->device));
    int rc = emit_if_needed(h);
    if (rc) return rc;
    const FilterView& v = h->v;
    const int64_t W = slot_words(h->d, v.npad, v.nseg);
    const int64_t span = v.npad > v.nseg ? v.npad : v.nseg;
    // a slot may be packed several times (a heavy theta-particle copied to many ranks): k can exceed
    // n_theta, so go in chunks of the index buffer's capacity
    for (int64_t k0 = 0; k0 < k; k0 += v.ntheta) {
        const int64_t kc = k - k0 < v.ntheta ? k - k0 : v.ntheta;
        HIPCHK(hipMemcpyAsync(h->d_perm, idx + k0, (size_t)kc * 4, hipMemcpyHostToDevice, h->stream));
        const dim3 grid((unsigned)((span + 255) / 256), (unsigned)kc);
        uint64_t* b = (uint64_t*)buf + (size_t)k0 * W;
        if (pack)
            hipLaunchKernelGGL((k_pack_slots<true>), grid, dim3(256), 0, h->stream, v, h->cur, h->d, h->d_perm, b);
        else
            hipLaunchKernelGGL((k_pack_slots<false>), grid, dim3(256), 0, h->stream, v, h->cur, h->d, h->d_perm, b);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return SMC_OK;
}
extern "C" int smc_pack_slots(smc_handle h, const int32_t* idx, int64_t k, void* device_buf) {
    return pack_unpack(h, idx, k, device_buf, true);
}
extern "C" int smc_unpack_slots(smc_handle h, const int32_t* idx, int64_t k, const void* device_buf) {
    return pack_unpack(h, idx, k, const_cast<void*>(device_buf), false);
}

extern "C" int smc_get_weights_raw(smc_handle h, uint64_t* C, double* m, uint64_t* S, uint64_t* S2hi, uint64_t* S2lo) {
    if (!h) return fail(SMC_EINVAL, "smc_get_weights_raw: NULL handle");
    if (!h->inited) return fail(SMC_ESTATE, "smc_get_weights_raw: filter not initialised");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const FilterView& v = h->v;
    const size_t np = (size_t)v.ntheta * v.npad * 8, ns = (size_t)v.ntheta * v.nseg * 8;
    const int c = h->cur;
    if (C) HIPCHK(hipMemcpy(C, v.C[c], np, hipMemcpyDeviceToHost));
    if (m) HIPCHK(hipMemcpy(m, v.segk[c], ns, hipMemcpyDeviceToHost));
    if (S) HIPCHK(hipMemcpy(S, v.segS[c], ns, hipMemcpyDeviceToHost));
    if (S2hi) HIPCHK(hipMemcpy(S2hi, v.segS2hi[c], ns, hipMemcpyDeviceToHost));
    if (S2lo) HIPCHK(hipMemcpy(S2lo, v.segS2lo[c], ns, hipMemcpyDeviceToHost));
    return SMC_OK;
}
