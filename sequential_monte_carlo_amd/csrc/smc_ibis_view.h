// smc_ibis_view.h -- what the kernels of the IBIS sampler share whatever the kind of row (smc_kalman_rows.h) a parameter particle
// filters: the view of the resident cloud, the map theta -> row, the reductions over a segment of 8 lanes, and the segment record
// of the outer reweight.  Inline device code only (no kernel): included by smc_ibis_kernels.h.
#pragma once
#include "smc_kalman_rows.h"
#include "smc_kernels.h"

namespace smc {

constexpr int IBIS_OSEG = 8;              // SMC_OUTER_SEG: entries per segment record of the outer reweight
constexpr int IBIS_NRAW = Lg1Row::NRAW;   // LinearModel row (A, B, Q, R, x0, sigma0)
constexpr int IBIS_THREADS = 64;          // one wave per workgroup: a cloud of a few hundred particles still spreads over the CUs
constexpr int IBIS_MAX_WINDOW = 64;

// Row::NRAW, Row::NX, Row::NS doubles per particle, Row the kind of row of the handle
struct IbisView {
    int64_t M;
    double* theta[2];     // [M][MAX_DTHETA]   (theta, raw) and (x, S, logZ, logw) are double-buffered separately:
    double* raw[2];       // [M][nraw]          a window leaves its end state in the other (x, S, logZ, logw) set,
    double* x[2];         // [M][nx]            a permutation gathers both
    double* S[2];         // [M][nS]
    double* logZ[2];      // [M]
    double* logw[2];      // [M]
};

// smc.model(theta) of a handle: row[k] = from[k] >= 0 ? theta[from[k]] : cst[k].  Long enough for either kind of row; a kernel
// reads the first Row::NRAW entries.  (The prior, d / family / par, is the handle's PmmhSpec.)
struct IbisRowMap {
    int from[LG2_NRAW];
    double cst[LG2_NRAW];
};
static_assert(Lg1Row::NRAW <= LG2_NRAW && Lg2Row::NRAW <= LG2_NRAW, "IbisRowMap holds the map of either kind of row");

// reductions over the 8 consecutive lanes of a segment (lane & ~7 .. lane | 7), result in every one of them: quad_perm
// [1,0,3,2], quad_perm [2,3,0,1] and row_half_mirror (lane i <-> 7 - i of each half row) as DPP moves
template <int CTRL>
__device__ __forceinline__ uint32_t seg8_move(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false);
}
template <int CTRL>
__device__ __forceinline__ uint64_t seg8_move64(uint64_t v) {
    return ((uint64_t)seg8_move<CTRL>((uint32_t)(v >> 32)) << 32) | seg8_move<CTRL>((uint32_t)v);
}
__device__ __forceinline__ int seg8_max(int v) {
    int o = (int)seg8_move<0xB1>((uint32_t)v); v = o > v ? o : v;
    o = (int)seg8_move<0x4E>((uint32_t)v); v = o > v ? o : v;
    o = (int)seg8_move<0x141>((uint32_t)v); v = o > v ? o : v;
    return v;
}
__device__ __forceinline__ uint64_t seg8_sum(uint64_t v) {
    v += seg8_move64<0xB1>(v);
    v += seg8_move64<0x4E>(v);
    v += seg8_move64<0x141>(v);
    return v;
}
__device__ __forceinline__ U128 seg8_sum128(U128 v) {
    v = add128(v, U128{seg8_move64<0xB1>(v.lo), seg8_move64<0xB1>(v.hi)});
    v = add128(v, U128{seg8_move64<0x4E>(v.lo), seg8_move64<0x4E>(v.hi)});
    v = add128(v, U128{seg8_move64<0x141>(v.lo), seg8_move64<0x141>(v.hi)});
    return v;
}

// the record (kb, S, S2hi, S2lo) of the calling lane's segment of reweight(logw) - the integers smc_host_outer_window computes
// from the same logw; rec_j: [nseg][4], the records of one step.  Every lane of the wave calls it; the first valid lane of a
// segment stores (a vector store).
__device__ __forceinline__ void ibis_outer_record(double logw, bool valid, int64_t m, uint64_t* rec_j) {
    const bool alive = valid && lw_alive(logw);
    double kd = 0.0;
    const double p = sp_exp_parts(alive ? logw : 0.0, kd);
    const int ki = alive ? (int)kd : -(1 << 30);
    const int kb = seg8_max(ki);
    const uint64_t q = alive ? fix_weight_i(p, ki - kb, FIX_BITS) : 0;
    const uint64_t Ssum = seg8_sum(q);
    const U128 s2 = seg8_sum128(sq128(q));
    if (valid && (threadIdx.x & (IBIS_OSEG - 1)) == 0) {
        uint64_t* r = rec_j + (size_t)(m / IBIS_OSEG) * 4;
        const bool live = kb != -(1 << 30);
        r[0] = d2bits(live ? (double)kb : -inf());
        r[1] = live ? Ssum : 0;
        r[2] = live ? s2.hi : 0;
        r[3] = live ? s2.lo : 0;
    }
}

}  // namespace smc
