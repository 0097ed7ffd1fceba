// smc_ibis.hip -- C ABI of the IBIS sampler (include/smc_hip.h "IBIS"; src/ibis.jl): the handle that keeps a cloud of
// parameter particles with their exact Kalman state on the device, and the launches of smc_ibis_kernels.h.
#include "smc_host.h"
#include "smc_ibis_kernels.h"
#include "smc_ibis_smooth_kernels.h"
#include "smc_theta_kernels.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

using namespace smc;

struct smc_ibis_s {
    uint32_t magic = 0x53494249u;   // "IBIS": the boundary type is void*, so a foreign pointer is at least noticed
    int device = 0;
    int predict_first = 0;
    uint32_t flags = 0;             // smc_ibis_set_flags: 0 or SMC_FLAG_NAN_MISSING (a NaN observation is a missing Kalman step)
    hipStream_t stream = nullptr;
    IbisView v{};                   // views of the two sets below, as the kernels take them
    int row_id = MODEL_LG1D;        // what a parameter particle filters: scalar LG1D rows (smc_ibis_create) or two-state MODEL_LG2D rows
    DevBlock d_theta[2], d_raw[2], d_x[2], d_S[2], d_logZ[2], d_logw[2];   // double [M][MAX_DTHETA] | [M][nraw] | [M][nx] | [M][nS] | [M] each
    int cp = 0, cs = 0;             // current (theta, raw) set and current (x, S, logZ, logw) set
    PmmhSpec spec{};                // d and the prior
    IbisRowMap map{};               // smc.model(theta): the first row_len(h) entries
    bool configured = false, have_theta = false;
    int64_t t = 0;                  // observations committed so far
    int win_k = 0;                  // steps of the pending window (its end state sits in set cs ^ 1); 0: none
    std::vector<double> win_y;
    // every block below is freed with the handle; those without a size here grow on demand (old block first)
    DevBlock d_y;                   // double [T] or [k]
    DevBlock d_lik;                 // double [k][M]
    DevBlock d_rec;                 // uint64_t [k][nseg][4]
    DevBlock d_a;                   // int32_t [M]
    DevBlock d_moved;               // unsigned char [M]
    DevBlock d_count;               // unsigned long long [1]
    DevBlock d_chol;                // double [MAX_DTHETA^2] | sq [IBIS_MAX_CHAIN]
    // summaries (smc_ibis_set_summaries / smc_ibis_summary): chunk records and scratch, rows of the last window
    bool summ_on = false;
    int summ_ahead = 0;
    DevBlock d_part;                                 // double [rows][IBIS_SUM_NCOL][nchunk]
    DevBlock d_srow;                                 // double [IBIS_MAX_WINDOW][IBIS_SUM_NOUT]
    DevBlock d_one;                                  // double [IBIS_SUM_NCOL][nchunk] | [IBIS_SUM_NOUT]: smc_ibis_summary
    double srow[IBIS_MAX_WINDOW * IBIS_SUM_NOUT];
    int srow_k = 0;                                  // rows of srow that are set
    // the resample-move loop on the device (smc_ibis_window_ess / smc_ibis_resample / smc_ibis_theta_moments)
    bool have_moved = false;                         // d_moved holds the mask of a rejuvenation
    DevBlock d_K;                                    // uint32_t [IBIS_MAX_WINDOW] biased K of every step of a window | [0] of the cloud
    DevBlock d_DR;                                   // unsigned long long [IBIS_MAX_WINDOW][2] (D, R) of every step
    DevBlock d_q;                                    // uint64_t [M] fixed-point weights | then the inclusive scan of cnt
    DevBlock d_seg;                                  // uint64_t [nseg] S | [nseg] Dcum | [ntile(M)] tile sums of the scans
    DevBlock d_skb;                                  // uint32_t [nseg] biased kb
    DevBlock d_cnt;                                  // int32_t [M] draws per particle
    DevBlock d_mpart;                                // double [THETA_MOM_NTRI][nchunk] chunk sums of the moments
    DevBlock d_mom;                                  // double [IBIS_MOM_N]
    // quantiles and histograms of the theta cloud (smc_ibis_theta_quantiles / _histogram; their weights take d_q, their K d_K[0])
    DevBlock d_tsel;                                 // uint64_t [THETA_SEL_WORDS] the select's state | [THETA_HIST_MAXBINS + 3] counts
    double rts_ms = -1.0;                            // device-event time of the kernels of the last smooth / sample_paths call
};
typedef smc_ibis_s* ibis_t;

namespace {
constexpr int IBIS_MAX_CHAIN = 64;

ibis_t as_ibis(void* p) {
    ibis_t h = (ibis_t)p;
    return (h && h->magic == 0x53494249u) ? h : nullptr;
}
unsigned grid_of(int64_t M) { return (unsigned)((M + IBIS_THREADS - 1) / IBIS_THREADS); }
// a handle of two-state rows: a particle holds Lg2Row::NRAW row entries, x [2] and the lower triangle S [3].  Asked for the
// lengths of its buffers, for what it refuses, and by the dispatcher below; every other line of this file serves both kinds.
bool two_state(const smc_ibis_s* h) { return h->row_id == MODEL_LG2D; }
size_t row_len(const smc_ibis_s* h) { return two_state(h) ? Lg2Row::NRAW : Lg1Row::NRAW; }
size_t x_len(const smc_ibis_s* h) { return two_state(h) ? Lg2Row::NX : Lg1Row::NX; }
size_t S_len(const smc_ibis_s* h) { return two_state(h) ? Lg2Row::NS : Lg1Row::NS; }
// what a two-state handle does not have (gaps, cloud summaries, the cloud's RTS smoother and its paths): SMC_EINVAL, handle unchanged
int refuse_two_state(const char* who, const char* what) {
    return fail(SMC_EINVAL, std::string(who) + ": " + what + " is not implemented for a handle of two-state rows (smc_ibis_create_rows with SMC_MODEL_LG2D)");
}

void release(ibis_t h) {   // (the blocks go with the handle)
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

// f(D), D = std::integral_constant<int, d>: the dimension of theta as a compile-time constant
template <class F>
void by_d(int d, F f) {
    switch (d) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    case 6: f(std::integral_constant<int, 6>{}); break;
    case 7: f(std::integral_constant<int, 7>{}); break;
    default: f(std::integral_constant<int, 8>{}); break;
    }
}
// The dispatcher of the kernels that are templates on the kind of row: f(Row{}, D, MISS) for the handle's kind, its d, and
// miss: the handle is flagged AND the observations of this launch hold a NaN - the MISS twin; else the kernels an unflagged handle
// runs.  A two-state handle has no flag (smc_ibis_set_flags refuses it), so MISS is instantiated for scalar rows only.
template <class F>
void by_row_d(const smc_ibis_s* h, bool miss, F f) {
    by_d(h->spec.d, [&](auto d) {
        if (two_state(h)) f(Lg2Row{}, d, std::false_type{});
        else if (miss) f(Lg1Row{}, d, std::true_type{});
        else f(Lg1Row{}, d, std::false_type{});
    });
}

void launch_init(ibis_t h) {
    by_row_d(h, false, [&](auto row, auto d, auto) {
        hipLaunchKernelGGL((k_ibis_init<decltype(row), decltype(d)::value>), dim3(grid_of(h->v.M)), dim3(IBIS_THREADS), 0, h->stream, h->v, h->cp,
                           h->cs, h->map);
    });
}
void launch_reset(ibis_t h) {
    by_row_d(h, false, [&](auto row, auto, auto) {
        hipLaunchKernelGGL((k_ibis_reset<decltype(row)>), dim3(grid_of(h->v.M)), dim3(IBIS_THREADS), 0, h->stream, h->v, h->cp, h->cs);
    });
}
// the gather through d_a into the other buffers (the caller flips cp and cs)
void launch_permute(ibis_t h) {
    by_row_d(h, false, [&](auto row, auto, auto) {
        hipLaunchKernelGGL((k_ibis_permute<decltype(row)>), dim3(grid_of(h->v.M)), dim3(IBIS_THREADS), 0, h->stream, h->v, h->cp, h->cs,
                           h->d_a.as<const int32_t>());
    });
}
void launch_rejuvenate(ibis_t h, bool miss, int64_t T, double xi, int chain, uint64_t move_seed) {
    by_row_d(h, miss, [&](auto row, auto d, auto m) {
        hipLaunchKernelGGL((k_ibis_rejuvenate<decltype(row), decltype(d)::value, decltype(m)::value>), dim3(grid_of(h->v.M)), dim3(IBIS_THREADS), 0,
                           h->stream, h->v, h->cp, h->cs, h->spec, h->map, h->d_y.as<double>(), T, h->predict_first, xi, h->d_chol.as<double>(),
                           h->d_chol.as<double>() + MAX_DTHETA * MAX_DTHETA, chain, move_seed, h->d_moved.as<unsigned char>(),
                           h->d_count.as<unsigned long long>());
    });
}
// rec: the segment records (RECORD; with them lik, optional); part: the chunk records of the summaries (SUMM: the handle records
// them, so it is one of scalar rows); both null: the steps alone
void launch_window(ibis_t h, bool miss, int dst, const double* d_y, int k, int predict0, double* lik, uint64_t* rec, double* part, int ahead) {
    by_row_d(h, miss, [&](auto row, auto, auto m) {
        using Row = decltype(row);
        auto go = [&](auto record, auto summ) {
            hipLaunchKernelGGL((k_ibis_window<Row, decltype(record)::value, decltype(summ)::value, decltype(m)::value>), dim3(grid_of(h->v.M)),
                               dim3(IBIS_THREADS), 0, h->stream, h->v, h->cp, h->cs, dst, d_y, k, predict0, lik, rec, part, ahead);
        };
        if constexpr (std::is_same_v<Row, Lg1Row>) {
            if (part) return go(std::true_type{}, std::true_type{});
        }
        if (rec) go(std::true_type{}, std::false_type{});
        else go(std::false_type{}, std::false_type{});
    });
}
void launch_rts_forward(hipStream_t st, bool miss, const double* raw, int64_t M, const double* d_y, int64_t T, int predict_first, double* xf,
                        double* Sf) {
    if (miss)
        hipLaunchKernelGGL((k_ibis_rts_forward<true>), dim3(grid_of(M)), dim3(IBIS_THREADS), 0, st, raw, M, d_y, T, predict_first, xf, Sf);
    else
        hipLaunchKernelGGL((k_ibis_rts_forward<false>), dim3(grid_of(M)), dim3(IBIS_THREADS), 0, st, raw, M, d_y, T, predict_first, xf, Sf);
}

// run `steps` observations from the committed state in place (no records): the prefix of a window that is kept, or a whole series
int steps_in_place(ibis_t h, const double* y, int64_t steps) {
    HIPCHK(h->d_y.grow((size_t)steps * 8));
    HIPCHK(hipMemcpyAsync(h->d_y.as<double>(), y, (size_t)steps * 8, hipMemcpyHostToDevice, h->stream));
    int64_t done = 0;
    while (done < steps) {   // (the kernel's step count is an int)
        const int k = (int)(steps - done > (1 << 20) ? (1 << 20) : steps - done);
        const int predict0 = (h->t + done > 0 || h->predict_first) ? 1 : 0;
        launch_window(h, kalman_has_gap(h->flags, y + done, k), h->cs, h->d_y.as<double>() + done, k, predict0, nullptr, nullptr, nullptr, 0);
        HIPCHK(hipGetLastError());
        done += k;
    }
    HIPCHK(hipStreamSynchronize(h->stream));   // (y is the caller's: the copy has to be over when the call returns)
    h->t += steps;
    return SMC_OK;
}
}  // namespace

extern "C" int smc_ibis_create(int64_t n_theta, uint64_t seed, int device, int predict_first, void* out) {
    return smc_ibis_create_rows(n_theta, seed, device, predict_first, MODEL_LG1D, out);
}

extern "C" int smc_ibis_create_rows(int64_t n_theta, uint64_t seed, int device, int predict_first, int row_id, void* out) {
    (void)seed;   // every random number of the device side is keyed by the move_seed of its call
    if (!out) return fail(SMC_EINVAL, "smc_ibis_create: NULL out");
    *(void**)out = nullptr;
    if (row_id != MODEL_LG1D && row_id != MODEL_LG2D) return fail(SMC_EINVAL, "smc_ibis_create_rows: row_id is SMC_MODEL_LG1D or SMC_MODEL_LG2D");
    if (n_theta < 1 || n_theta > ((int64_t)1 << 30)) return fail(SMC_EINVAL, "smc_ibis_create: 1 <= n_theta <= 2^30");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(SMC_EHIP, "smc_ibis_create: no HIP device");
    if (device < 0 || device >= ndev) return fail(SMC_EINVAL, "smc_ibis_create: bad device");
    HIPCHK(hipSetDevice(device));
    ibis_t h = new (std::nothrow) smc_ibis_s();
    if (!h) return fail(SMC_ENOMEM, "smc_ibis_create: out of host memory");
    h->device = device;
    h->predict_first = predict_first ? 1 : 0;
    h->v.M = n_theta;
    h->row_id = row_id;
    const size_t M = (size_t)n_theta;
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    for (int b = 0; b < 2 && e == hipSuccess; ++b) {
        if (e == hipSuccess) e = h->d_theta[b].grow(M * MAX_DTHETA * 8);
        if (e == hipSuccess) e = h->d_raw[b].grow(M * row_len(h) * 8);
        if (e == hipSuccess) e = h->d_x[b].grow(M * x_len(h) * 8);
        if (e == hipSuccess) e = h->d_S[b].grow(M * S_len(h) * 8);
        if (e == hipSuccess) e = h->d_logZ[b].grow(M * 8);
        if (e == hipSuccess) e = h->d_logw[b].grow(M * 8);
        h->v.theta[b] = h->d_theta[b].as<double>(); h->v.raw[b] = h->d_raw[b].as<double>(); h->v.x[b] = h->d_x[b].as<double>();
        h->v.S[b] = h->d_S[b].as<double>(); h->v.logZ[b] = h->d_logZ[b].as<double>(); h->v.logw[b] = h->d_logw[b].as<double>();
    }
    if (e == hipSuccess) e = h->d_a.grow(M * 4);
    if (e == hipSuccess) e = h->d_moved.grow(M);
    if (e == hipSuccess) e = h->d_count.grow(8);
    if (e == hipSuccess) e = h->d_chol.grow((MAX_DTHETA * MAX_DTHETA + IBIS_MAX_CHAIN) * 8);
    if (e == hipSuccess) e = h->d_srow.grow(IBIS_MAX_WINDOW * IBIS_SUM_NOUT * 8);
    if (e == hipSuccess) e = h->d_K.grow(IBIS_MAX_WINDOW * 4);
    if (e == hipSuccess) e = h->d_DR.grow(IBIS_MAX_WINDOW * 2 * 8);
    if (e == hipSuccess) e = h->d_mom.grow(IBIS_MOM_N * 8);
    if (e != hipSuccess) {
        release(h);
        return fail(e == hipErrorOutOfMemory ? SMC_ENOMEM : SMC_EHIP, std::string("smc_ibis_create: ") + hipGetErrorString(e));
    }
    *(void**)out = h;
    return SMC_OK;
}

extern "C" int smc_ibis_destroy(void* hp) {
    ibis_t h = as_ibis(hp);
    if (!h) return fail(SMC_EINVAL, "smc_ibis_destroy: not an IBIS handle");
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    h->magic = 0;
    release(h);
    return SMC_OK;
}

extern "C" int smc_ibis_configure(void* hp, int d_theta, const int32_t* prior_family, const double* prior_par, const int32_t* raw_from,
                                  const double* raw_const) {
    ibis_t h = as_ibis(hp);
    if (!h) return fail(SMC_EINVAL, "smc_ibis_configure: not an IBIS handle");
    if (!prior_family || !prior_par || !raw_from || !raw_const) return fail(SMC_EINVAL, "smc_ibis_configure: NULL argument");
    if (d_theta < 1 || d_theta > MAX_DTHETA) return fail(SMC_EINVAL, "smc_ibis_configure: 1 <= d_theta <= 8");
    PmmhSpec sp{};
    sp.d = d_theta;
    for (int i = 0; i < d_theta; ++i) {
        if (prior_family[i] < PRIOR_UNIFORM || prior_family[i] > PRIOR_LOGNORMAL)
            return fail(SMC_EINVAL, "smc_ibis_configure: unknown prior family " + std::to_string(prior_family[i]));
        sp.family[i] = prior_family[i];
        for (int k = 0; k < PRIOR_NPAR; ++k) sp.par[i][k] = prior_par[(size_t)i * PRIOR_NPAR + k];
    }
    IbisRowMap map{};
    for (size_t k = 0; k < row_len(h); ++k) {
        if (raw_from[k] >= d_theta) return fail(SMC_EINVAL, "smc_ibis_configure: raw_from index out of range");
        map.from[k] = raw_from[k];
        map.cst[k] = raw_const[k];
    }
    h->spec = sp;
    h->map = map;
    h->configured = true;
    h->have_theta = false;
    h->win_k = 0;
    return SMC_OK;
}

extern "C" int smc_ibis_set_theta(void* hp, const double* theta) {
    ibis_t h = as_ibis(hp);
    if (!h || !theta) return fail(SMC_EINVAL, "smc_ibis_set_theta: bad argument");
    if (!h->configured) return fail(SMC_ESTATE, "smc_ibis_set_theta: smc_ibis_configure has not been called");
    HIPCHK(hipSetDevice(h->device));
    const size_t M = (size_t)h->v.M;
    const int d = h->spec.d;
    std::vector<double> pad(M * MAX_DTHETA, 0.0);
    for (size_t m = 0; m < M; ++m)
        for (int i = 0; i < d; ++i) pad[m * MAX_DTHETA + i] = theta[m * d + i];
    HIPCHK(hipMemcpyAsync(h->v.theta[h->cp], pad.data(), pad.size() * 8, hipMemcpyHostToDevice, h->stream));
    launch_init(h);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    h->have_theta = true;
    h->t = 0;
    h->win_k = 0;
    h->srow_k = 0;
    h->have_moved = false;
    return SMC_OK;
}

// the launches of a window of k steps from the committed state: the records go to d_rec, lik (optional) to d_lik, the rows of
// the summaries (when recording) to srow.  Nothing is waited for.
static int enqueue_window(ibis_t h, const char* who, const double* y, int k, bool lik) {
    if (!h->have_theta) return fail(SMC_ESTATE, std::string(who) + ": smc_ibis_set_theta has not been called");
    if (k < 1 || k > IBIS_MAX_WINDOW) return fail(SMC_EINVAL, std::string(who) + ": 1 <= k <= 64");
    HIPCHK(hipSetDevice(h->device));
    h->win_k = 0;
    const size_t M = (size_t)h->v.M, nseg = (M + IBIS_OSEG - 1) / IBIS_OSEG;
    HIPCHK(h->d_y.grow((size_t)k * 8));
    HIPCHK(h->d_rec.grow((size_t)k * nseg * 4 * 8));
    if (lik) HIPCHK(h->d_lik.grow((size_t)k * M * 8));
    const size_t nchunk = grid_of(h->v.M);
    h->srow_k = 0;
    if (h->summ_on) HIPCHK(h->d_part.grow((size_t)k * IBIS_SUM_NCOL * nchunk * 8));
    HIPCHK(hipMemcpyAsync(h->d_y.as<double>(), y, (size_t)k * 8, hipMemcpyHostToDevice, h->stream));
    const bool miss = kalman_has_gap(h->flags, y, k);
    const int predict0 = (h->t > 0 || h->predict_first) ? 1 : 0;
    // with summaries: the same steps, and the chunk records of the summaries after each; then one workgroup per row combines them
    launch_window(h, miss, h->cs ^ 1, h->d_y.as<double>(), k, predict0, lik ? h->d_lik.as<double>() : nullptr, h->d_rec.as<uint64_t>(),
                  h->summ_on ? h->d_part.as<double>() : nullptr, h->summ_ahead);
    HIPCHK(hipGetLastError());
    if (h->summ_on) {
        hipLaunchKernelGGL(k_ibis_sum_combine, dim3((unsigned)k), dim3(IBIS_SUM_CTHREADS), 0, h->stream, h->d_part.as<double>(), (int64_t)nchunk,
                           h->d_srow.as<double>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h->srow, h->d_srow.as<double>(), (size_t)k * IBIS_SUM_NOUT * 8, hipMemcpyDeviceToHost, h->stream));
    }
    return SMC_OK;
}
// the window is pending: smc_ibis_commit may keep a prefix of it
static void window_pending(ibis_t h, const double* y, int k) {
    h->win_y.assign(y, y + k);
    h->win_k = k;
    if (h->summ_on) h->srow_k = k;
}

extern "C" int smc_ibis_window(void* hp, const double* y, int k, double* lik, uint64_t* rec) {
    ibis_t h = as_ibis(hp);
    if (!h || !y || !rec) return fail(SMC_EINVAL, "smc_ibis_window: bad argument");
    if (const int rc = enqueue_window(h, "smc_ibis_window", y, k, lik != nullptr)) return rc;
    const size_t M = (size_t)h->v.M, nseg = (M + IBIS_OSEG - 1) / IBIS_OSEG;
    HIPCHK(hipMemcpyAsync(rec, h->d_rec.as<uint64_t>(), (size_t)k * nseg * 32, hipMemcpyDeviceToHost, h->stream));
    if (lik) HIPCHK(hipMemcpyAsync(lik, h->d_lik.as<double>(), (size_t)k * M * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    window_pending(h, y, k);
    return SMC_OK;
}

// smc_ibis_window with the walk's three integers per step reduced on the device: k x 20 bytes come back instead of the records
extern "C" int smc_ibis_window_ess(void* hp, const double* y, int k, double ess_min, double* ess_out, int* j_out) {
    ibis_t h = as_ibis(hp);
    if (!h || !y || !ess_out || !j_out) return fail(SMC_EINVAL, "smc_ibis_window_ess: bad argument");
    if (const int rc = enqueue_window(h, "smc_ibis_window_ess", y, k, false)) return rc;
    const int64_t M = h->v.M, nseg = (M + IBIS_OSEG - 1) / IBIS_OSEG;
    const int SH = table_shift_extra(nseg * IBIS_OSEG);
    int64_t gx = (nseg + IBIS_RED_THREADS - 1) / IBIS_RED_THREADS;
    gx = gx > 128 ? 128 : gx;
    HIPCHK(hipMemsetAsync(h->d_K.as<uint32_t>(), 0, (size_t)k * 4, h->stream));
    HIPCHK(hipMemsetAsync(h->d_DR.as<unsigned long long>(), 0, (size_t)k * 16, h->stream));
    hipLaunchKernelGGL(k_ibis_rec_kmax, dim3((unsigned)gx, (unsigned)k), dim3(IBIS_RED_THREADS), 0, h->stream, h->d_rec.as<uint64_t>(), nseg, h->d_K.as<uint32_t>());
    hipLaunchKernelGGL(k_ibis_rec_sums, dim3((unsigned)gx, (unsigned)k), dim3(IBIS_RED_THREADS), 0, h->stream, h->d_rec.as<uint64_t>(), nseg, SH, h->d_K.as<uint32_t>(),
                       h->d_DR.as<unsigned long long>());
    HIPCHK(hipGetLastError());
    uint32_t Kb[IBIS_MAX_WINDOW];
    unsigned long long DR[IBIS_MAX_WINDOW * 2];
    HIPCHK(hipMemcpyAsync(Kb, h->d_K.as<uint32_t>(), (size_t)k * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(DR, h->d_DR.as<unsigned long long>(), (size_t)k * 16, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    int j = 0;
    while (j < k) {          // smc_host_outer_walk
        double logmu, ess;
        combine_outputs(ibis_unbias_k(Kb[j]), DR[2 * j], DR[2 * j + 1], SH, M, logmu, ess);
        ess_out[j++] = ess;
        if (ess < ess_min) break;
    }
    *j_out = j;
    window_pending(h, y, k);
    return SMC_OK;
}

extern "C" int smc_ibis_set_summaries(void* hp, int on, int ahead) {
    ibis_t h = as_ibis(hp);
    if (!h) return fail(SMC_EINVAL, "smc_ibis_set_summaries: not an IBIS handle");
    if (two_state(h)) return refuse_two_state("smc_ibis_set_summaries", "the summary of the cloud");
    if (ahead != 0 && ahead != 1) return fail(SMC_EINVAL, "smc_ibis_set_summaries: ahead is 0 or 1");
    h->summ_on = on != 0;
    h->summ_ahead = ahead;
    h->srow_k = 0;
    return SMC_OK;
}

// SMC_FLAG_NAN_MISSING for the handle: a series is filtered under one rule from its first step, so only at t = 0 with no window
// pending
extern "C" int smc_ibis_set_flags(void* hp, uint32_t flags) {
    ibis_t h = as_ibis(hp);
    if (!h) return fail(SMC_EINVAL, "smc_ibis_set_flags: not an IBIS handle");
    if (flags & ~SMC_FLAG_NAN_MISSING) return fail(SMC_EINVAL, "smc_ibis_set_flags: flags is 0 or SMC_FLAG_NAN_MISSING");
    if (flags && two_state(h)) return refuse_two_state("smc_ibis_set_flags", "SMC_FLAG_NAN_MISSING (the missing Kalman step)");
    if (h->t != 0 || h->win_k > 0)
        return fail(SMC_ESTATE, "smc_ibis_set_flags: observations have been taken (or a window is pending): the flag is set at t = 0");
    h->flags = flags;
    return SMC_OK;
}

extern "C" int smc_ibis_get_flags(void* hp, uint32_t* flags) {
    ibis_t h = as_ibis(hp);
    if (!h || !flags) return fail(SMC_EINVAL, "smc_ibis_get_flags: bad argument");
    *flags = h->flags;
    return SMC_OK;
}

extern "C" int smc_ibis_get_summaries(void* hp, int j, double* out) {
    ibis_t h = as_ibis(hp);
    if (!h || !out) return fail(SMC_EINVAL, "smc_ibis_get_summaries: bad argument");
    if (two_state(h)) return refuse_two_state("smc_ibis_get_summaries", "the summary of the cloud");
    if (j < 0 || j > h->srow_k) return fail(SMC_ESTATE, "smc_ibis_get_summaries: the last window recorded fewer steps (is recording on?)");
    memcpy(out, h->srow, (size_t)j * IBIS_SUM_NOUT * 8);
    return SMC_OK;
}

extern "C" int smc_ibis_summary(void* hp, int ahead, double* out) {
    ibis_t h = as_ibis(hp);
    if (!h || !out) return fail(SMC_EINVAL, "smc_ibis_summary: bad argument");
    if (two_state(h)) return refuse_two_state("smc_ibis_summary", "the summary of the cloud");
    if (ahead != 0 && ahead != 1) return fail(SMC_EINVAL, "smc_ibis_summary: ahead is 0 or 1");
    if (!h->have_theta) return fail(SMC_ESTATE, "smc_ibis_summary: smc_ibis_set_theta has not been called");
    HIPCHK(hipSetDevice(h->device));
    const size_t nchunk = grid_of(h->v.M);
    // (a buffer of its own: the rows of a pending window stay intact)
    HIPCHK(h->d_one.grow((IBIS_SUM_NCOL * nchunk + IBIS_SUM_NOUT) * 8));
    double* d_one = h->d_one.as<double>();
    hipLaunchKernelGGL(k_ibis_sum_chunks, dim3(grid_of(h->v.M)), dim3(IBIS_THREADS), 0, h->stream, h->v, h->cp, h->cs, ahead, d_one);
    hipLaunchKernelGGL(k_ibis_sum_combine, dim3(1), dim3(IBIS_SUM_CTHREADS), 0, h->stream, d_one, (int64_t)nchunk,
                       d_one + IBIS_SUM_NCOL * nchunk);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d_one + IBIS_SUM_NCOL * nchunk, IBIS_SUM_NOUT * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return SMC_OK;
}

// The same specification on the host (no GPU): rows [M][6] = (A, B, Q, R, x0, sigma0), x, S, logw [M]
extern "C" int smc_host_ibis_summary(const double* rows, const double* x, const double* S, const double* logw, int64_t M, int ahead,
                                     double* out) {
    if (!rows || !x || !S || !logw || !out || M < 1) return fail(SMC_EINVAL, "smc_host_ibis_summary: bad argument");
    if (ahead != 0 && ahead != 1) return fail(SMC_EINVAL, "smc_host_ibis_summary: ahead is 0 or 1");
    const int64_t nchunk = (M + IBIS_SUM_CHUNK - 1) / IBIS_SUM_CHUNK;
    std::vector<double> rec((size_t)nchunk * IBIS_SUM_NF);
    for (int64_t c = 0; c < nchunk; ++c) {
        double p[IBIS_SUM_CHUNK], u[IBIS_SUM_CHUNK], ym[IBIS_SUM_CHUNK], vm[IBIS_SUM_CHUNK], xs[IBIS_SUM_CHUNK], Ss[IBIS_SUM_CHUNK];
        double t[7][IBIS_SUM_CHUNK];
        int k[IBIS_SUM_CHUNK], kc = IBIS_SUM_DEADK;
        for (int l = 0; l < IBIS_SUM_CHUNK; ++l) {
            const int64_t m = c * IBIS_SUM_CHUNK + l;
            const bool valid = m < M;
            const int64_t mm = valid ? m : M - 1;
            const double* r = rows + mm * IBIS_NRAW;
            xs[l] = x[mm];
            Ss[l] = S[mm];
            p[l] = ibis_sum_parts(logw[mm], valid, k[l]);
            kc = k[l] > kc ? k[l] : kc;
            ibis_obs_moments(r[0], r[1], r[2], r[3], xs[l], Ss[l], ahead != 0, ym[l], vm[l]);
        }
        int ls = -1;
        for (int l = 0; l < IBIS_SUM_CHUNK; ++l) {
            u[l] = ibis_sum_u(p[l], k[l], kc);
            if (u[l] > 0.0 && (ls < 0 || u[l] > u[ls])) ls = l;
        }
        const double cy = ls >= 0 ? ym[ls] : 0.0, cx = ls >= 0 ? xs[ls] : 0.0;
        for (int l = 0; l < IBIS_SUM_CHUNK; ++l) {
            double tl[7];
            ibis_sum_terms(u[l], ym[l], vm[l], xs[l], Ss[l], cy, cx, tl);
            for (int i = 0; i < 7; ++i) t[i][l] = tl[i];
        }
        for (int i = 0; i < 7; ++i)      // lane 0 of the butterfly: the balanced tree over neighbours
            for (int s = 1; s < IBIS_SUM_CHUNK; s <<= 1)
                for (int l = 0; l < IBIS_SUM_CHUNK; l += 2 * s) t[i][l] = t[i][l] + t[i][l + s];
        double* r = rec.data() + (size_t)c * IBIS_SUM_NF;
        r[ISF_KC] = kc == IBIS_SUM_DEADK ? -inf() : (double)kc;
        r[ISF_W] = t[0][0]; r[ISF_CY] = cy; r[ISF_DY] = t[1][0]; r[ISF_V] = t[2][0]; r[ISF_MY] = t[3][0];
        r[ISF_CX] = cx; r[ISF_DX] = t[4][0]; r[ISF_SX] = t[5][0]; r[ISF_MX] = t[6][0];
    }
    double K = -inf(), D = 0.0;
    for (int64_t c = 0; c < nchunk; ++c) K = rec[(size_t)c * IBIS_SUM_NF] > K ? rec[(size_t)c * IBIS_SUM_NF] : K;
    for (int64_t c = 0; c < nchunk; ++c) {
        const double* r = rec.data() + (size_t)c * IBIS_SUM_NF;
        D = D + ibis_sum_factor(K, r[ISF_KC], r[ISF_W]) * r[ISF_W];
    }
    double a[4] = {0.0, 0.0, 0.0, 0.0}, b[2] = {0.0, 0.0};
    for (int64_t c = 0; c < nchunk; ++c) {
        const double* r = rec.data() + (size_t)c * IBIS_SUM_NF;
        double ac[4];
        ibis_sum_first(r, ibis_sum_factor(K, r[ISF_KC], r[ISF_W]), D, ac);
        for (int i = 0; i < 4; ++i) a[i] = a[i] + ac[i];
    }
    for (int64_t c = 0; c < nchunk; ++c) {
        const double* r = rec.data() + (size_t)c * IBIS_SUM_NF;
        double bc[2];
        ibis_sum_second(r, ibis_sum_factor(K, r[ISF_KC], r[ISF_W]), D, a[0], a[2], bc);
        for (int i = 0; i < 2; ++i) b[i] = b[i] + bc[i];
    }
    const bool live = D > 0.0;
    const double nan = bits2d(0x7ff8000000000000ULL);
    out[0] = live ? a[0] : nan; out[1] = live ? a[1] : nan; out[2] = live ? b[0] : nan;
    out[3] = live ? a[2] : nan; out[4] = live ? a[3] : nan; out[5] = live ? b[1] : nan;
    out[6] = K; out[7] = D;
    return SMC_OK;
}

extern "C" int smc_ibis_commit(void* hp, int j) {
    ibis_t h = as_ibis(hp);
    if (!h) return fail(SMC_EINVAL, "smc_ibis_commit: not an IBIS handle");
    if (h->win_k < 1) return fail(SMC_ESTATE, "smc_ibis_commit: no pending window");
    if (j < 0 || j > h->win_k) return fail(SMC_EINVAL, "smc_ibis_commit: j outside the window");
    HIPCHK(hipSetDevice(h->device));
    const int k = h->win_k;
    h->win_k = 0;
    if (j == k) {            // the window's end state is the new state
        h->cs ^= 1;
        h->t += k;
        return SMC_OK;
    }
    if (j == 0) return SMC_OK;
    return steps_in_place(h, h->win_y.data(), j);   // the same arithmetic on the same operands: the bits of the window's first j steps
}

extern "C" int smc_ibis_filter(void* hp, const double* y, int64_t T) {
    ibis_t h = as_ibis(hp);
    if (!h || !y || T < 1) return fail(SMC_EINVAL, "smc_ibis_filter: bad argument");
    if (!h->have_theta) return fail(SMC_ESTATE, "smc_ibis_filter: smc_ibis_set_theta has not been called");
    HIPCHK(hipSetDevice(h->device));
    h->win_k = 0;
    launch_reset(h);
    HIPCHK(hipGetLastError());
    h->t = 0;
    return steps_in_place(h, y, T);
}

extern "C" int smc_ibis_permute(void* hp, const int32_t* a) {
    ibis_t h = as_ibis(hp);
    if (!h || !a) return fail(SMC_EINVAL, "smc_ibis_permute: bad argument");
    if (!h->have_theta) return fail(SMC_ESTATE, "smc_ibis_permute: smc_ibis_set_theta has not been called");
    const int64_t M = h->v.M;
    for (int64_t m = 0; m < M; ++m)
        if (a[m] < 0 || a[m] >= M) return fail(SMC_EINVAL, "smc_ibis_permute: ancestor index out of range");
    HIPCHK(hipSetDevice(h->device));
    h->win_k = 0;
    HIPCHK(hipMemcpyAsync(h->d_a.as<int32_t>(), a, (size_t)M * 4, hipMemcpyHostToDevice, h->stream));
    launch_permute(h);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    h->cp ^= 1;
    h->cs ^= 1;
    return SMC_OK;
}

extern "C" int smc_ibis_set_logw(void* hp, const double* logw) {
    ibis_t h = as_ibis(hp);
    if (!h || !logw) return fail(SMC_EINVAL, "smc_ibis_set_logw: bad argument");
    if (!h->have_theta) return fail(SMC_ESTATE, "smc_ibis_set_logw: smc_ibis_set_theta has not been called");
    HIPCHK(hipSetDevice(h->device));
    h->win_k = 0;
    HIPCHK(hipMemcpyAsync(h->v.logw[h->cs], logw, (size_t)h->v.M * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return SMC_OK;
}

extern "C" int smc_ibis_rejuvenate(void* hp, const double* y, int64_t T, double xi, const double* chol, const double* scales, int chain,
                                   uint64_t move_seed, int64_t* accepted, uint8_t* moved) {
    ibis_t h = as_ibis(hp);
    if (!h || !y || !chol || !scales) return fail(SMC_EINVAL, "smc_ibis_rejuvenate: bad argument");
    if (!h->have_theta) return fail(SMC_ESTATE, "smc_ibis_rejuvenate: smc_ibis_set_theta has not been called");
    if (T < 1 || chain < 0 || chain > IBIS_MAX_CHAIN) return fail(SMC_EINVAL, "smc_ibis_rejuvenate: T >= 1, 0 <= chain <= 64");
    HIPCHK(hipSetDevice(h->device));
    h->win_k = 0;
    const int d = h->spec.d;
    double par[MAX_DTHETA * MAX_DTHETA + IBIS_MAX_CHAIN] = {0.0};
    for (int i = 0; i < d * d; ++i) par[i] = chol[i];
    for (int c = 0; c < chain; ++c) par[MAX_DTHETA * MAX_DTHETA + c] = sqrt(scales[c]);
    HIPCHK(h->d_y.grow((size_t)T * 8));
    HIPCHK(hipMemcpyAsync(h->d_y.as<double>(), y, (size_t)T * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_chol.as<double>(), par, sizeof(par), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(h->d_count.as<unsigned long long>(), 0, 8, h->stream));
    launch_rejuvenate(h, kalman_has_gap(h->flags, y, T), T, xi, chain, move_seed);
    HIPCHK(hipGetLastError());
    unsigned long long n = 0;
    HIPCHK(hipMemcpyAsync(&n, h->d_count.as<unsigned long long>(), 8, hipMemcpyDeviceToHost, h->stream));
    if (moved) HIPCHK(hipMemcpyAsync(moved, h->d_moved.as<unsigned char>(), (size_t)h->v.M, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (accepted) *accepted = (int64_t)n;
    h->have_moved = true;
    return SMC_OK;
}

extern "C" int smc_ibis_get_moved(void* hp, uint8_t* moved) {
    ibis_t h = as_ibis(hp);
    if (!h || !moved) return fail(SMC_EINVAL, "smc_ibis_get_moved: bad argument");
    if (!h->have_moved) return fail(SMC_ESTATE, "smc_ibis_get_moved: smc_ibis_rejuvenate has not been called");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(moved, h->d_moved.as<unsigned char>(), (size_t)h->v.M, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return SMC_OK;
}

namespace {
// inclusive scan of f(0 .. n) into out [n]; tsum: ceil(n / IBIS_RED_THREADS) words of scratch
template <class F>
void launch_scan(ibis_t h, F f, int64_t n, uint64_t* tsum, uint64_t* out) {
    const int64_t ntile = (n + IBIS_RED_THREADS - 1) / IBIS_RED_THREADS;
    hipLaunchKernelGGL((k_ibis_scan_sums<F>), dim3((unsigned)ntile), dim3(IBIS_RED_THREADS), 0, h->stream, f, n, tsum);
    hipLaunchKernelGGL(k_ibis_scan_offsets, dim3(1), dim3(IBIS_RED_THREADS), 0, h->stream, tsum, ntile);
    hipLaunchKernelGGL((k_ibis_scan_tiles<F>), dim3((unsigned)ntile), dim3(IBIS_RED_THREADS), 0, h->stream, f, n, (const uint64_t*)tsum, out);
}
template <int D>
void launch_moments(ibis_t h, int weighted, int64_t nchunk) {
    const int64_t M = h->v.M;
    const int ntri = D * (D + 1) / 2;
    hipLaunchKernelGGL((k_ibis_mom_chunks<D, 1>), dim3((unsigned)nchunk), dim3(IBIS_THREADS), 0, h->stream, h->v, h->cp, h->cs, weighted,
                       h->d_K.as<const uint32_t>(), h->d_mom.as<const double>(), h->d_mpart.as<double>());
    hipLaunchKernelGGL(k_ibis_mom_combine, dim3(1), dim3(IBIS_THREADS), 0, h->stream, h->d_mpart.as<const double>(), D, nchunk,
                       h->d_mom.as<double>() + IBIS_MOM_MEAN, weighted ? 0 : 1, (double)M, weighted, h->d_mom.as<const double>());
    hipLaunchKernelGGL((k_ibis_mom_chunks<D, 2>), dim3((unsigned)nchunk), dim3(IBIS_THREADS), 0, h->stream, h->v, h->cp, h->cs, weighted,
                       h->d_K.as<const uint32_t>(), h->d_mom.as<const double>(), h->d_mpart.as<double>());
    hipLaunchKernelGGL(k_ibis_mom_combine, dim3(1), dim3(IBIS_THREADS), 0, h->stream, h->d_mpart.as<const double>(), ntri, nchunk,
                       h->d_mom.as<double>() + IBIS_MOM_COV, weighted ? 0 : 1, (double)(M - 1), weighted, h->d_mom.as<const double>());
}
}  // namespace

// resample!(ibis) without the host: the ancestors of smc_host_outer_resample(logw, M, M, seed) for the committed logw, bit for
// bit (steps 1-6 of its specification as kernels), then the gather of smc_ibis_permute with `a` left on the device
extern "C" int smc_ibis_resample(void* hp, uint64_t seed, int32_t* a_out) {
    ibis_t h = as_ibis(hp);
    if (!h) return fail(SMC_EINVAL, "smc_ibis_resample: not an IBIS handle");
    if (!h->have_theta) return fail(SMC_ESTATE, "smc_ibis_resample: smc_ibis_set_theta has not been called");
    HIPCHK(hipSetDevice(h->device));
    h->win_k = 0;
    const int64_t M = h->v.M, nseg = (M + IBIS_OSEG - 1) / IBIS_OSEG, ntile = (M + IBIS_RED_THREADS - 1) / IBIS_RED_THREADS;
    const int SH = table_shift_extra(nseg * IBIS_OSEG);
    // (each buffer on its own: a call that ran out of memory half way leaves the rest to the next one)
    HIPCHK(h->d_q.grow((size_t)M * 8));
    HIPCHK(h->d_seg.grow((size_t)(2 * nseg + ntile) * 8));
    HIPCHK(h->d_skb.grow((size_t)nseg * 4));
    HIPCHK(h->d_cnt.grow((size_t)M * 4));
    uint64_t *sS = h->d_seg.as<uint64_t>(), *Dcum = sS + nseg, *tsum = sS + 2 * nseg;
    HIPCHK(hipMemsetAsync(h->d_K.as<uint32_t>(), 0, 4, h->stream));
    HIPCHK(hipMemsetAsync(h->d_cnt.as<int32_t>(), 0, (size_t)M * 4, h->stream));
    hipLaunchKernelGGL(k_ibis_rs_weights, dim3(grid_of(M)), dim3(IBIS_THREADS), 0, h->stream, h->v, h->cs, h->d_q.as<uint64_t>(), h->d_skb.as<uint32_t>(), sS, h->d_K.as<uint32_t>());
    launch_scan(h, IbisSegQ{h->d_skb.as<uint32_t>(), sS, h->d_K.as<uint32_t>(), SH}, nseg, tsum, Dcum);
    hipLaunchKernelGGL(k_ibis_rs_draw, dim3(grid_of((M + 1) / 2)), dim3(IBIS_THREADS), 0, h->stream, M, seed, h->d_q.as<const uint64_t>(),
                       h->d_skb.as<const uint32_t>(), h->d_K.as<const uint32_t>(), SH, (const uint64_t*)Dcum, nseg, h->d_cnt.as<int32_t>());
    launch_scan(h, IbisCount{h->d_cnt.as<int32_t>()}, M, tsum, h->d_q.as<uint64_t>());          // (the weights are spent: their array takes the scan of cnt)
    hipLaunchKernelGGL(k_ibis_rs_expand, dim3(grid_of(M)), dim3(IBIS_THREADS), 0, h->stream, M, h->d_q.as<const uint64_t>(), h->d_a.as<int32_t>());
    launch_permute(h);
    HIPCHK(hipGetLastError());
    if (a_out) HIPCHK(hipMemcpyAsync(a_out, h->d_a.as<int32_t>(), (size_t)M * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->cp ^= 1;
    h->cs ^= 1;
    return SMC_OK;
}

// mean [d] and cov [d][d] of the committed theta cloud (smc_spec.h "moments of the theta cloud"); (d + d^2) doubles come back
extern "C" int smc_ibis_theta_moments(void* hp, int weighted, double* mean, double* cov) {
    ibis_t h = as_ibis(hp);
    if (!h || !mean || !cov) return fail(SMC_EINVAL, "smc_ibis_theta_moments: bad argument");
    if (weighted != 0 && weighted != 1) return fail(SMC_EINVAL, "smc_ibis_theta_moments: weighted is 0 or 1");
    if (!h->have_theta) return fail(SMC_ESTATE, "smc_ibis_theta_moments: smc_ibis_set_theta has not been called");
    HIPCHK(hipSetDevice(h->device));
    const int64_t nchunk = grid_of(h->v.M);
    const int d = h->spec.d;
    HIPCHK(h->d_mpart.grow((size_t)THETA_MOM_NTRI * (size_t)nchunk * 8));
    if (weighted) {
        HIPCHK(hipMemsetAsync(h->d_K.as<uint32_t>(), 0, 4, h->stream));
        hipLaunchKernelGGL(k_ibis_kmax, dim3((unsigned)nchunk), dim3(IBIS_THREADS), 0, h->stream, h->v, h->cs, h->d_K.as<uint32_t>());
        hipLaunchKernelGGL(k_ibis_mom_w, dim3((unsigned)nchunk), dim3(IBIS_THREADS), 0, h->stream, h->v, h->cs, h->d_K.as<const uint32_t>(),
                           h->d_mpart.as<double>());
        hipLaunchKernelGGL(k_ibis_mom_combine, dim3(1), dim3(IBIS_THREADS), 0, h->stream, h->d_mpart.as<const double>(), 1, nchunk, h->d_mom.as<double>(), 0,
                           0.0, 0, h->d_mom.as<const double>());
    }
    by_d(d, [&](auto D) { launch_moments<decltype(D)::value>(h, weighted, nchunk); });
    HIPCHK(hipGetLastError());
    double mom[IBIS_MOM_N];
    HIPCHK(hipMemcpyAsync(mom, h->d_mom.as<double>(), sizeof(mom), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int i = 0; i < d; ++i) {
        mean[i] = mom[IBIS_MOM_MEAN + i];
        for (int j = 0; j <= i; ++j) cov[i * d + j] = cov[j * d + i] = mom[IBIS_MOM_COV + i * (i + 1) / 2 + j];
    }
    return SMC_OK;
}

namespace {
// What the two calls below share: the refusals, then K, q [M] (in d_q) and W of the committed logw enqueued on the stream.
// groups: the workgroups of a streaming pass.  SMC_THETA_GROUPS caps them (a test knob: no result depends on it).
int theta_weights_enqueue(ibis_t h, const char* who, ThetaSel& st, unsigned& groups) {
    if (!h->have_theta) return fail(SMC_ESTATE, std::string(who) + ": smc_ibis_set_theta has not been called");
    if (h->win_k > 0) return fail(SMC_ESTATE, std::string(who) + ": a window is pending (smc_ibis_commit first)");
    HIPCHK(hipSetDevice(h->device));
    const int64_t M = h->v.M;
    HIPCHK(h->d_q.grow((size_t)M * 8));
    HIPCHK(h->d_tsel.grow((THETA_SEL_WORDS + THETA_HIST_MAXBINS + 3) * 8));
    st = theta_sel_carve(h->d_tsel.as<uint64_t>());
    int64_t cap = THETA_MAX_GROUPS;
    if (const char* e = getenv("SMC_THETA_GROUPS")) cap = atoll(e);
    cap = cap < 1 ? 1 : cap > THETA_MAX_GROUPS ? THETA_MAX_GROUPS : cap;
    const int64_t tiles = (M + IBIS_RED_THREADS - 1) / IBIS_RED_THREADS;
    groups = (unsigned)(tiles < cap ? tiles : cap);
    HIPCHK(hipMemsetAsync(h->d_K.as<uint32_t>(), 0, 4, h->stream));
    HIPCHK(hipMemsetAsync(st.W, 0, 8, h->stream));
    // (the grid of the passes, not one wave per workgroup: atomics on one word are served one after the other, 16 K of them in 188 us)
    hipLaunchKernelGGL(k_ibis_kmax, dim3(groups), dim3(IBIS_RED_THREADS), 0, h->stream, h->v, h->cs, h->d_K.as<uint32_t>());
    hipLaunchKernelGGL(k_theta_weights, dim3(groups), dim3(IBIS_RED_THREADS), 0, h->stream, h->v, h->cs, h->d_K.as<const uint32_t>(), h->d_q.as<uint64_t>(),
                       st.W);
    return SMC_OK;
}
template <int D>
hipError_t launch_theta_select(ibis_t h, unsigned groups, int np, const ThetaLevels& lv, const ThetaSel& st) {
    const size_t lds = (size_t)D * np * THETA_SEL_BINS * 8;
    if (lds > 48 * 1024) {   // (up to 128 KiB at d = np = 8: one workgroup per CU)
        const hipError_t e = hipFuncSetAttribute((const void*)k_theta_digits<D>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_theta_pick, dim3(1), dim3(IBIS_RED_THREADS), 0, h->stream, D, np, -1, lv, st);
    for (int pass = 0; pass < THETA_SEL_PASSES; ++pass) {
        hipLaunchKernelGGL((k_theta_digits<D>), dim3(groups), dim3(IBIS_RED_THREADS), lds, h->stream, (const double*)h->v.theta[h->cp],
                           h->d_q.as<const uint64_t>(), h->v.M, np, pass, st);
        hipLaunchKernelGGL(k_theta_pick, dim3(1), dim3(IBIS_RED_THREADS), 0, h->stream, D, np, pass, lv, st);
    }
    return hipGetLastError();
}
}  // namespace

// weighted quantiles of every coordinate of the committed theta cloud (smc_spec.h "quantiles and histograms of the theta cloud"):
// a radix select on the device, d np doubles come back
extern "C" int smc_ibis_theta_quantiles(void* hp, const double* p, int np, double* out) {
    ibis_t h = as_ibis(hp);
    if (!h || !p || !out) return fail(SMC_EINVAL, "smc_ibis_theta_quantiles: bad argument");
    if (np < 1 || np > QMAX) return fail(SMC_EINVAL, "smc_ibis_theta_quantiles: 1 <= np <= 8");
    ThetaLevels lv{};
    for (int j = 0; j < np; ++j) {
        if (!(p[j] >= 0.0 && p[j] <= 1.0)) return fail(SMC_EINVAL, "smc_ibis_theta_quantiles: levels must lie in [0, 1]");
        lv.p64[j] = prob_to_u64(p[j]);
    }
    ThetaSel st;
    unsigned groups = 0;
    if (const int rc = theta_weights_enqueue(h, "smc_ibis_theta_quantiles", st, groups)) return rc;
    const int d = h->spec.d;
    hipError_t e = hipSuccess;
    by_d(d, [&](auto D) { e = launch_theta_select<decltype(D)::value>(h, groups, np, lv, st); });
    HIPCHK(e);
    double res[THETA_SEL_SLOTS];
    HIPCHK(hipMemcpyAsync(res, st.out, sizeof(res), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < np; ++j) out[i * np + j] = res[i * QMAX + j];
    return SMC_OK;
}

// the weighted histogram of one coordinate of the committed theta cloud: counts [nbins + 3] = under | bins | over | nan, and W
extern "C" int smc_ibis_theta_histogram(void* hp, int component, double lo, double hi, int nbins, uint64_t* counts, uint64_t* W) {
    ibis_t h = as_ibis(hp);
    if (!h || !counts || !W) return fail(SMC_EINVAL, "smc_ibis_theta_histogram: bad argument");
    if (nbins < 1 || nbins > THETA_HIST_MAXBINS) return fail(SMC_EINVAL, "smc_ibis_theta_histogram: 1 <= nbins <= 4096");
    if (!theta_hist_range_ok(lo, hi)) return fail(SMC_EINVAL, "smc_ibis_theta_histogram: lo < hi, both finite (and hi - lo finite)");
    if (h->have_theta && (component < 0 || component >= h->spec.d)) return fail(SMC_EINVAL, "smc_ibis_theta_histogram: component outside [0, d_theta)");
    ThetaSel st;
    unsigned groups = 0;
    if (const int rc = theta_weights_enqueue(h, "smc_ibis_theta_histogram", st, groups)) return rc;
    unsigned long long* d_counts = (unsigned long long*)(h->d_tsel.as<uint64_t>() + THETA_SEL_WORDS);
    HIPCHK(hipMemsetAsync(d_counts, 0, (size_t)(nbins + 3) * 8, h->stream));
    hipLaunchKernelGGL(k_theta_hist, dim3(groups), dim3(IBIS_RED_THREADS), 0, h->stream, (const double*)h->v.theta[h->cp], h->d_q.as<const uint64_t>(), h->v.M,
                       component, lo, hi, (double)nbins / (hi - lo), nbins, d_counts);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(counts, d_counts, (size_t)(nbins + 3) * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(W, st.W, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return SMC_OK;
}

extern "C" int smc_ibis_get(void* hp, double* theta, double* x, double* S, double* logZ, double* logw) {
    ibis_t h = as_ibis(hp);
    if (!h) return fail(SMC_EINVAL, "smc_ibis_get: not an IBIS handle");
    if (!h->have_theta) return fail(SMC_ESTATE, "smc_ibis_get: smc_ibis_set_theta has not been called");
    HIPCHK(hipSetDevice(h->device));
    const size_t M = (size_t)h->v.M;
    std::vector<double> pad;
    if (theta) {
        pad.resize(M * MAX_DTHETA);
        HIPCHK(hipMemcpyAsync(pad.data(), h->v.theta[h->cp], pad.size() * 8, hipMemcpyDeviceToHost, h->stream));
    }
    if (x) HIPCHK(hipMemcpyAsync(x, h->v.x[h->cs], M * x_len(h) * 8, hipMemcpyDeviceToHost, h->stream));
    if (S) HIPCHK(hipMemcpyAsync(S, h->v.S[h->cs], M * S_len(h) * 8, hipMemcpyDeviceToHost, h->stream));
    if (logZ) HIPCHK(hipMemcpyAsync(logZ, h->v.logZ[h->cs], M * 8, hipMemcpyDeviceToHost, h->stream));
    if (logw) HIPCHK(hipMemcpyAsync(logw, h->v.logw[h->cs], M * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (theta) {
        const int d = h->spec.d;
        for (size_t m = 0; m < M; ++m)
            for (int i = 0; i < d; ++i) theta[m * d + i] = pad[m * MAX_DTHETA + i];
    }
    return SMC_OK;
}

// ---- the RTS smoother of the cloud and its backward-sampled paths (smc_spec.h "the RTS smoother of an IBIS cloud") -------------
// Everything these calls need on the device is allocated by the call and freed before it returns: the handle is read only.
namespace {
struct CallEvents {   // the bracket of a call's kernels on the handle's stream
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~CallEvents() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    hipError_t create() { const hipError_t e = hipEventCreate(&e0); return e != hipSuccess ? e : hipEventCreate(&e1); }
    double ms() const { float f = 0.0f; return hipEventElapsedTime(&f, e0, e1) == hipSuccess ? (double)f : -1.0; }
};
constexpr int64_t RTS_MAX_T = (int64_t)1 << 31;   // the step index is a 32-bit word of the Philox counter
}  // namespace

extern "C" int smc_ibis_smooth(void* hp, const double* y, int64_t T, double* out, double* xs, double* Ps) {
    ibis_t h = as_ibis(hp);
    if (!h || !y || !out) return fail(SMC_EINVAL, "smc_ibis_smooth: bad argument");
    if (two_state(h)) return refuse_two_state("smc_ibis_smooth", "the RTS smoother of the cloud (smc_kalman2_smooth smooths rows)");
    if (T < 1 || T > RTS_MAX_T) return fail(SMC_EINVAL, "smc_ibis_smooth: 1 <= T <= 2^31");
    if (!h->have_theta) return fail(SMC_ESTATE, "smc_ibis_smooth: smc_ibis_set_theta has not been called");
    if (h->win_k > 0) return fail(SMC_ESTATE, "smc_ibis_smooth: a window is pending (smc_ibis_commit first)");
    HIPCHK(hipSetDevice(h->device));
    const size_t M = (size_t)h->v.M, nchunk = grid_of(h->v.M), sT = (size_t)T;
    const size_t b_out = sT * IBIS_SUM_NOUT * 8;
    OffsetPlan plan;
    const size_t o_y = plan.take(sT * 8), o_xf = plan.take(sT * M * 8), o_Sf = plan.take(sT * M * 8);
    const size_t o_part = plan.take(sT * IBIS_SUM_NCOL * nchunk * 8), o_out = plan.take(b_out);
    DevBlock blk;   // (a local block: freed when the call returns)
    if (const hipError_t e = blk.grow(plan.bytes)) return alloc_fail("smc_ibis_smooth", e);
    char* const base = blk.as<char>();
    double *d_y = (double*)(base + o_y), *d_xf = (double*)(base + o_xf), *d_Sf = (double*)(base + o_Sf);
    double *d_part = (double*)(base + o_part), *d_out = (double*)(base + o_out);
    const bool store = xs != nullptr || Ps != nullptr;
    CallEvents ev;
    HIPCHK(ev.create());
    HIPCHK(hipMemcpyAsync(d_y, y, sT * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipEventRecord(ev.e0, h->stream));
    launch_rts_forward(h->stream, kalman_has_gap(h->flags, y, T), h->v.raw[h->cp], h->v.M, d_y, T, h->predict_first, d_xf, d_Sf);
    if (store)
        hipLaunchKernelGGL((k_ibis_rts_backward<true, true>), dim3(grid_of(h->v.M)), dim3(IBIS_THREADS), 0, h->stream,
                           (const double*)h->v.raw[h->cp], (const double*)h->v.logw[h->cs], h->v.M, T, d_xf, d_Sf, d_part);
    else
        hipLaunchKernelGGL((k_ibis_rts_backward<true, false>), dim3(grid_of(h->v.M)), dim3(IBIS_THREADS), 0, h->stream,
                           (const double*)h->v.raw[h->cp], (const double*)h->v.logw[h->cs], h->v.M, T, d_xf, d_Sf, d_part);
    hipLaunchKernelGGL(k_ibis_sum_combine, dim3((unsigned)T), dim3(IBIS_SUM_CTHREADS), 0, h->stream, d_part, (int64_t)nchunk, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev.e1, h->stream));
    HIPCHK(hipMemcpyAsync(out, d_out, b_out, hipMemcpyDeviceToHost, h->stream));
    if (xs) HIPCHK(hipMemcpyAsync(xs, d_xf, sT * M * 8, hipMemcpyDeviceToHost, h->stream));
    if (Ps) HIPCHK(hipMemcpyAsync(Ps, d_Sf, sT * M * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->rts_ms = ev.ms();
    return SMC_OK;
}

extern "C" int smc_ibis_sample_paths(void* hp, const double* y, int64_t T, int64_t Mp, uint64_t path_seed, const int32_t* which,
                                     double* paths) {
    ibis_t h = as_ibis(hp);
    if (!h || !y || !which || !paths) return fail(SMC_EINVAL, "smc_ibis_sample_paths: bad argument");
    if (two_state(h)) return refuse_two_state("smc_ibis_sample_paths", "backward sampling of paths");
    if (T < 1 || T > RTS_MAX_T) return fail(SMC_EINVAL, "smc_ibis_sample_paths: 1 <= T <= 2^31");
    if (Mp < 1 || Mp > ((int64_t)1 << 30)) return fail(SMC_EINVAL, "smc_ibis_sample_paths: 1 <= Mp <= 2^30");
    if (!h->have_theta) return fail(SMC_ESTATE, "smc_ibis_sample_paths: smc_ibis_set_theta has not been called");
    if (h->win_k > 0) return fail(SMC_ESTATE, "smc_ibis_sample_paths: a window is pending (smc_ibis_commit first)");
    for (int64_t p = 0; p < Mp; ++p)
        if (which[p] < 0 || which[p] >= h->v.M) return fail(SMC_EINVAL, "smc_ibis_sample_paths: which entry outside [0, n_theta)");
    HIPCHK(hipSetDevice(h->device));
    const size_t sM = (size_t)Mp, sT = (size_t)T;
    OffsetPlan plan;
    const size_t o_y = plan.take(sT * 8), o_w = plan.take(sM * 4), o_paths = plan.take(sT * sM * 8), o_Sf = plan.take(sT * sM * 8);
    DevBlock blk;
    if (const hipError_t e = blk.grow(plan.bytes)) return alloc_fail("smc_ibis_sample_paths", e);
    char* const base = blk.as<char>();
    double* d_y = (double*)(base + o_y);
    int32_t* d_w = (int32_t*)(base + o_w);
    double *d_paths = (double*)(base + o_paths), *d_Sf = (double*)(base + o_Sf);
    HIPCHK(hipMemcpyAsync(d_y, y, sT * 8, hipMemcpyHostToDevice, h->stream));
    CallEvents ev;
    HIPCHK(ev.create());
    HIPCHK(hipMemcpyAsync(d_w, which, sM * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipEventRecord(ev.e0, h->stream));
    if (kalman_has_gap(h->flags, y, T))
        hipLaunchKernelGGL((k_ibis_rts_paths<true>), dim3(grid_of(Mp)), dim3(IBIS_THREADS), 0, h->stream, (const double*)h->v.raw[h->cp],
                           (const int32_t*)d_w, Mp, (const double*)d_y, T, h->predict_first, path_seed, d_paths, d_Sf);
    else
        hipLaunchKernelGGL((k_ibis_rts_paths<false>), dim3(grid_of(Mp)), dim3(IBIS_THREADS), 0, h->stream, (const double*)h->v.raw[h->cp],
                           (const int32_t*)d_w, Mp, (const double*)d_y, T, h->predict_first, path_seed, d_paths, d_Sf);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev.e1, h->stream));
    HIPCHK(hipMemcpyAsync(paths, d_paths, sT * sM * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->rts_ms = ev.ms();
    return SMC_OK;
}

extern "C" int smc_ibis_last_elapsed_ms(void* hp, double* ms) {
    ibis_t h = as_ibis(hp);
    if (!h || !ms) return fail(SMC_EINVAL, "smc_ibis_last_elapsed_ms: bad argument");
    if (h->rts_ms < 0.0) return fail(SMC_ESTATE, "smc_ibis_last_elapsed_ms: no smc_ibis_smooth / smc_ibis_sample_paths call has completed");
    *ms = h->rts_ms;
    return SMC_OK;
}

// the per-row half of smc_ibis_smooth without a handle: the counterpart of smc_kalman_log_likelihood
extern "C" int smc_kalman_smooth_flags(const double* raw, int64_t n_theta, const double* y, int64_t T, int predict_first, double* xs,
                                       double* Ps, int device, uint32_t flags) {
    if (flags & ~SMC_FLAG_NAN_MISSING) return fail(SMC_EINVAL, "smc_kalman_smooth: flags is 0 or SMC_FLAG_NAN_MISSING");
    if (!raw || !y || !xs || !Ps) return fail(SMC_EINVAL, "smc_kalman_smooth: bad argument");
    if (n_theta < 1 || n_theta > ((int64_t)1 << 30) || T < 1 || T > RTS_MAX_T) return fail(SMC_EINVAL, "smc_kalman_smooth: 1 <= n_theta <= 2^30, 1 <= T <= 2^31");
    DeviceCall c;   // (its memory is the call's own: counted while it runs, freed when it returns)
    if (const int rc = c.begin("smc_kalman_smooth", device)) return rc;
    const size_t b_y = (size_t)T * 8, b_raw = (size_t)n_theta * IBIS_NRAW * 8, b_rec = (size_t)T * (size_t)n_theta * 8;
    const size_t o_y = c.take(b_y), o_raw = c.take(b_raw), o_xf = c.take(b_rec), o_Sf = c.take(b_rec);
    if (const int rc = c.use_own()) return rc;
    double *d_raw = c.at<double>(o_raw), *d_xf = c.at<double>(o_xf), *d_Sf = c.at<double>(o_Sf);
    HIPCHK(c.upload(o_y, y, b_y));
    HIPCHK(c.upload(o_raw, raw, b_raw));
    launch_rts_forward(c.stream, kalman_has_gap(flags, y, T), d_raw, n_theta, c.at<double>(o_y), T, predict_first ? 1 : 0, d_xf, d_Sf);
    hipLaunchKernelGGL((k_ibis_rts_backward<false, true>), dim3(grid_of(n_theta)), dim3(IBIS_THREADS), 0, c.stream, (const double*)d_raw,
                       (const double*)nullptr, n_theta, T, d_xf, d_Sf, (double*)nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(c.download(xs, o_xf, b_rec));
    HIPCHK(c.download(Ps, o_Sf, b_rec));
    HIPCHK(c.finish());
    return SMC_OK;
}
extern "C" int smc_kalman_smooth(const double* raw, int64_t n_theta, const double* y, int64_t T, int predict_first, double* xs, double* Ps,
                                 int device) {
    return smc_kalman_smooth_flags(raw, n_theta, y, T, predict_first, xs, Ps, device, 0);
}

namespace {
// one step of a host twin: the flag read once per series (a NaN without it takes the ordinary step)
inline double host_kalman_step(bool miss, const double* r, bool predict, double y, double& x, double& S) {
    return miss ? kalman_step_gaps<true>(r[0], r[1], r[2], r[3], predict, y, x, S) : kalman_step(r[0], r[1], r[2], r[3], predict, y, x, S);
}
}  // namespace

// The step loop of one row on the host (no GPU): the filtered record and the value of every step, so that every array the
// device calls produce has a host array to be compared with.  row [6], y [T] -> xf, Sf, lik [T] (each optional)
extern "C" int smc_host_kalman_steps(const double* row, const double* y, int64_t T, int predict_first, uint32_t flags, double* xf,
                                     double* Sf, double* lik) {
    if (!row || !y || T < 1) return fail(SMC_EINVAL, "smc_host_kalman_steps: bad argument");
    if (flags & ~SMC_FLAG_NAN_MISSING) return fail(SMC_EINVAL, "smc_host_kalman_steps: flags is 0 or SMC_FLAG_NAN_MISSING");
    const bool miss = (flags & SMC_FLAG_NAN_MISSING) != 0;
    double x = row[4], S = row[5];
    for (int64_t t = 0; t < T; ++t) {
        const double l = host_kalman_step(miss, row, t > 0 || predict_first != 0, y[t], x, S);
        if (xf) xf[t] = x;
        if (Sf) Sf[t] = S;
        if (lik) lik[t] = l;
    }
    return SMC_OK;
}

// The same specification on the host (no GPU), the same bits.  xf, Sf: the filtered record the backward pass ran over.
extern "C" int smc_host_ibis_smooth_flags(const double* rows, const double* logw, int64_t M, const double* y, int64_t T, int predict_first,
                                          double* out, double* xs, double* Ps, double* xf, double* Sf, uint32_t flags) {
    if (flags & ~SMC_FLAG_NAN_MISSING) return fail(SMC_EINVAL, "smc_host_ibis_smooth: flags is 0 or SMC_FLAG_NAN_MISSING");
    const bool miss = (flags & SMC_FLAG_NAN_MISSING) != 0;
    if (!rows || !logw || !y || !out || M < 1) return fail(SMC_EINVAL, "smc_host_ibis_smooth: bad argument");
    if (T < 1 || T > RTS_MAX_T) return fail(SMC_EINVAL, "smc_host_ibis_smooth: 1 <= T <= 2^31");
    const size_t sM = (size_t)M, sT = (size_t)T;
    std::vector<double> bx, bP;
    if (!xs) { bx.resize(sT * sM); xs = bx.data(); }
    if (!Ps) { bP.resize(sT * sM); Ps = bP.data(); }
    for (size_t m = 0; m < sM; ++m) {
        const double* r = rows + m * IBIS_NRAW;
        double x = r[4], S = r[5];
        for (size_t t = 0; t < sT; ++t) {
            (void)host_kalman_step(miss, r, t > 0 || predict_first != 0, y[t], x, S);
            xs[t * sM + m] = x;
            Ps[t * sM + m] = S;
            if (xf) xf[t * sM + m] = x;
            if (Sf) Sf[t * sM + m] = S;
        }
        double a = x, P = S;
        for (size_t t = sT - 1; t-- > 0;) {
            rts_back(r[0], r[2], xs[t * sM + m], Ps[t * sM + m], a, P);
            xs[t * sM + m] = a;
            Ps[t * sM + m] = P;
        }
    }
    for (size_t t = 0; t < sT; ++t)
        if (const int rc = smc_host_ibis_summary(rows, xs + t * sM, Ps + t * sM, logw, M, 0, out + t * IBIS_SUM_NOUT)) return rc;
    return SMC_OK;
}
extern "C" int smc_host_ibis_smooth(const double* rows, const double* logw, int64_t M, const double* y, int64_t T, int predict_first,
                                    double* out, double* xs, double* Ps, double* xf, double* Sf) {
    return smc_host_ibis_smooth_flags(rows, logw, M, y, T, predict_first, out, xs, Ps, xf, Sf, 0);
}

extern "C" int smc_host_ibis_sample_paths_flags(const double* rows, int64_t M, const double* y, int64_t T, int predict_first, int64_t Mp,
                                                uint64_t path_seed, const int32_t* which, double* paths, double* z, uint32_t flags) {
    if (flags & ~SMC_FLAG_NAN_MISSING) return fail(SMC_EINVAL, "smc_host_ibis_sample_paths: flags is 0 or SMC_FLAG_NAN_MISSING");
    const bool miss = (flags & SMC_FLAG_NAN_MISSING) != 0;
    if (!rows || !y || !which || !paths || M < 1) return fail(SMC_EINVAL, "smc_host_ibis_sample_paths: bad argument");
    if (T < 1 || T > RTS_MAX_T) return fail(SMC_EINVAL, "smc_host_ibis_sample_paths: 1 <= T <= 2^31");
    if (Mp < 1 || Mp > ((int64_t)1 << 30)) return fail(SMC_EINVAL, "smc_host_ibis_sample_paths: 1 <= Mp <= 2^30");
    for (int64_t p = 0; p < Mp; ++p)
        if (which[p] < 0 || which[p] >= M) return fail(SMC_EINVAL, "smc_host_ibis_sample_paths: which entry outside [0, M)");
    const size_t sM = (size_t)Mp, sT = (size_t)T;
    std::vector<double> Sf(sT);
    for (int64_t p = 0; p < Mp; ++p) {
        const double* r = rows + (size_t)which[p] * IBIS_NRAW;
        const uint32_t stream = (uint32_t)which[p];
        double x = r[4], S = r[5];
        for (size_t t = 0; t < sT; ++t) {
            (void)host_kalman_step(miss, r, t > 0 || predict_first != 0, y[t], x, S);
            paths[t * sM + (size_t)p] = x;
            Sf[t] = S;
        }
        double zt = rts_normal(path_seed, p, stream, (uint32_t)(T - 1));
        double xp = rts_path_last(x, S, zt);
        paths[(sT - 1) * sM + (size_t)p] = xp;
        if (z) z[(sT - 1) * sM + (size_t)p] = zt;
        for (size_t t = sT - 1; t-- > 0;) {
            zt = rts_normal(path_seed, p, stream, (uint32_t)t);
            xp = rts_path_back(r[0], r[2], paths[t * sM + (size_t)p], Sf[t], xp, zt);
            paths[t * sM + (size_t)p] = xp;
            if (z) z[t * sM + (size_t)p] = zt;
        }
    }
    return SMC_OK;
}
extern "C" int smc_host_ibis_sample_paths(const double* rows, int64_t M, const double* y, int64_t T, int predict_first, int64_t Mp,
                                          uint64_t path_seed, const int32_t* which, double* paths, double* z) {
    return smc_host_ibis_sample_paths_flags(rows, M, y, T, predict_first, Mp, path_seed, which, paths, z, 0);
}
