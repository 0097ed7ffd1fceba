// smc_slot_kernels.h -- the state of whole filters moved as data (state read-back, outer resample!, the accept copy, pack /
// unpack).  Included by smc_capi_slots.hip only (non-template kernels: one translation unit).
#pragma once
#include "smc_kernels.h"

namespace smc {

// ---------------------------------------------------------------------------------------------
// dense normalised weights w_i (normalize()'s `w`, particles.jl:11) for smc_get_state
// ---------------------------------------------------------------------------------------------
__global__ void k_dense_weights(FilterView v, int cur, double* w /*[ntheta][n]*/) {
    const int th = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= v.n) return;
    const double K = v.last_K[th];
    const uint64_t Dtot = v.last_D[th];
    const int b = (int)(i / v.seg), j = (int)(i % v.seg);
    const uint64_t* C = v.C[cur] + (size_t)th * v.npad;
    const uint64_t q = C[i] - (j ? C[i - 1] : 0);
    const double dk = K - v.segk[cur][(size_t)th * v.nseg + b];
    const double sc = (dk >= 0.0 && dk < 900.0) ? pow2i(-48 - (int)dk) : 0.0;
    const double Dd = (double)Dtot * pow2i(v.SH - 48);
    w[(size_t)th * v.n + i] = Dtot ? ((double)q * sc) / Dd : 0.0;
}

// ---------------------------------------------------------------------------------------------
// outer resample!(smc) (smc_samplers.jl:74-84): theta slot m <- slot a[m], value copy of the
// whole filter state (x cloud, C, segment records, logZ).  grid (blocks, ntheta)
// ---------------------------------------------------------------------------------------------
__global__ void k_permute(FilterView v, int cur, int d, const int32_t* a, const double* logZ_src) {
    const int th = blockIdx.y, src = a[th], nxt = cur ^ 1;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < v.npad) {
        for (int c = 0; c < d; ++c)
            v.x[nxt][((size_t)c * v.ntheta + th) * v.npad + i] = v.x[cur][((size_t)c * v.ntheta + src) * v.npad + i];
        v.C[nxt][(size_t)th * v.npad + i] = v.C[cur][(size_t)src * v.npad + i];
    }
    if (i < v.nseg) {
        const size_t o = (size_t)th * v.nseg + i, s = (size_t)src * v.nseg + i;
        v.segk[nxt][o] = v.segk[cur][s];
        v.segS[nxt][o] = v.segS[cur][s];
        v.segS2hi[nxt][o] = v.segS2hi[cur][s];
        v.segS2lo[nxt][o] = v.segS2lo[cur][s];
    }
    if (i == 0) v.logZ[th] = logZ_src[src];
}

// slot <-> packed buffer.  Packed slot layout in 8-byte words:
//   x [d][npad] | C [npad] | kb,S,S2hi,S2lo [4][nseg] | logZ,last_logmu,last_ess,last_K,last_D [5]   (+ pad to even)
__host__ __device__ inline int64_t slot_words(int d, int64_t npad, int nseg) {
    const int64_t w = (int64_t)(d + 1) * npad + 4 * (int64_t)nseg + 5;
    return (w + 1) & ~(int64_t)1;
}
template <bool PACK>
__global__ void k_pack_slots(FilterView v, int cur, int d, const int32_t* idx, uint64_t* buf) {
    const int s = blockIdx.y, th = idx[s];
    const int64_t W = slot_words(d, v.npad, v.nseg);
    uint64_t* b = buf + (size_t)s * W;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    auto mv = [&](uint64_t* slot_word, uint64_t* dev_word) {
        if (PACK) *slot_word = *dev_word; else *dev_word = *slot_word;
    };
    if (i < v.npad) {
        for (int c = 0; c < d; ++c) mv(b + (size_t)c * v.npad + i, (uint64_t*)(v.x[cur] + ((size_t)c * v.ntheta + th) * v.npad + i));
        mv(b + (size_t)d * v.npad + i, v.C[cur] + (size_t)th * v.npad + i);
    }
    uint64_t* r = b + (size_t)(d + 1) * v.npad;
    if (i < v.nseg) {
        const size_t o = (size_t)th * v.nseg + i;
        mv(r + i, (uint64_t*)(v.segk[cur] + o));
        mv(r + v.nseg + i, v.segS[cur] + o);
        mv(r + 2 * (size_t)v.nseg + i, v.segS2hi[cur] + o);
        mv(r + 3 * (size_t)v.nseg + i, v.segS2lo[cur] + o);
    }
    if (i == 0) {
        uint64_t* t = r + 4 * (size_t)v.nseg;
        mv(t + 0, (uint64_t*)(v.logZ + th));
        mv(t + 1, (uint64_t*)(v.last_logmu + th));
        mv(t + 2, (uint64_t*)(v.last_ess + th));
        mv(t + 3, (uint64_t*)(v.last_K + th));
        mv(t + 4, v.last_D + th);
    }
}

// accept step: slot th of dst <- slot th of src where mask[th]   grid (blocks, ntheta)
__global__ void k_copy_slots(FilterView dst, int dcur, FilterView src, int scur, int d, const unsigned char* mask) {
    const int th = blockIdx.y;
    if (!mask[th]) return;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < dst.npad) {
        for (int c = 0; c < d; ++c)
            dst.x[dcur][((size_t)c * dst.ntheta + th) * dst.npad + i] = src.x[scur][((size_t)c * src.ntheta + th) * src.npad + i];
        dst.C[dcur][(size_t)th * dst.npad + i] = src.C[scur][(size_t)th * src.npad + i];
    }
    if (i < dst.nseg) {
        const size_t o = (size_t)th * dst.nseg + i;
        dst.segk[dcur][o] = src.segk[scur][o];
        dst.segS[dcur][o] = src.segS[scur][o];
        dst.segS2hi[dcur][o] = src.segS2hi[scur][o];
        dst.segS2lo[dcur][o] = src.segS2lo[scur][o];
    }
    if (i == 0) {
        dst.logZ[th] = src.logZ[th];
        dst.last_logmu[th] = src.last_logmu[th];
        dst.last_ess[th] = src.last_ess[th];
        dst.last_K[th] = src.last_K[th];
        dst.last_D[th] = src.last_D[th];
    }
}

}  // namespace smc
