// smc_spec.h -- numerical specification of the particle-filter hot path, host + device.
//
// Everything a particle ever computes is defined here with IEEE-754 binary64 +,-,*,/,sqrt,
// explicit fma() and integer arithmetic only, so that a gfx950 lane and a host core produce
// the same bits (DESIGN.md "Numerical specification").  Compile with -ffp-contract=off.
//
// Reference semantics being implemented (charlesknipp/sequential_monte_carlo @ v1):
//   rand(Normal(mu,sigma)), logpdf(Normal(mu,sigma),y)   src/particles.jl:97-98,123-124
//   model methods                                        src/state_space_models.jl:87-109,233-259
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SMC_HD __host__ __device__ __forceinline__

namespace smc {

// ---- model ids (C ABI values) ---------------------------------------------------------
constexpr int MODEL_LG1D = 1;    // UnivariateLinearGaussian  ssm.jl:74-109
constexpr int MODEL_SV1D = 2;    // stochastic volatility (SURVEY A7'; obs template ssm.jl:244-247)
constexpr int MODEL_UCSV3D = 3;  // UCSV                      ssm.jl:215-263
constexpr int MODEL_UCSV_RB = 4;  // UCSV with the trend integrated out: a scalar Kalman filter inside every particle ("marginal families")
constexpr int NPARAM = 8;        // padded row length of raw / derived parameter tables

constexpr int FIX_BITS = 48;     // q = rint(p * 2^(48 + k - kb)),  exp(logw) = p * 2^k
constexpr int MAX_SEG = 8192;
constexpr uint32_t SIM_STREAM = 0xFFFFFFFFu;
constexpr uint32_t SLOT_RESAMPLE = 0u;   // within-segment pick of child j
constexpr uint32_t SLOT_NORMAL0 = 1u;    // slots 1..nz: state normals (nz = model_nz: d, but 2 for UCSV_RB)
constexpr uint32_t SLOT_OBS = 8u;        // simulate(): observation noise
constexpr uint32_t SLOT_COUNT = 9u;      // segment pick of draw i (multi-segment filters)
constexpr uint32_t SLOT_SYS = 10u;       // the one uniform of a systematic resampling step (opt-in)
constexpr uint32_t SLOT_BREAK = 16u;     // block break points: 16+2i normal, 17+2i uniform, i < 8; pair = block
constexpr uint32_t SLOT_PMMH_Z = 32u;    // PMMH proposal normals of a parameter particle: pair k holds z[2k], z[2k+1]
constexpr uint32_t SLOT_PMMH_U = 33u;    // the uniform of its accept test
constexpr uint32_t SLOT_COND = 38u;      // the retained slot of a conditional step ("the conditional particle filter" below), pair 0
constexpr uint32_t SLOT_OUTER = 34u;     // the pick numbers of resample!(smc) / resample!(ibis), stream OUTER_STREAM
constexpr uint32_t OUTER_STREAM = 0xFFFFFFFEu;   // Philox stream id of the outer level (theta particles use 0 .. M-1, simulate() 0xFFFFFFFF)
constexpr int MAX_DTHETA = 8;            // parameter dimension of the samplers (SMC_MAX_DTHETA)

constexpr double HALF_LOG2PI = 0x1.d67f1c864beb5p-1;
constexpr double INV_LN2 = 0x1.71547652b82fep+0;
constexpr double LN2_HI = 0x1.62e42fee00000p-1;
constexpr double LN2_LO = 0x1.a39ef35793c76p-33;
constexpr double SQRT2 = 0x1.6a09e667f3bcdp+0;
constexpr double PIO4 = 0x1.921fb54442d18p-1;
constexpr double TWO_M53 = 0x1p-53;
constexpr double TWO_M48 = 0x1p-48;
constexpr double TWO_P48 = 0x1p+48;
constexpr double TWO_M96 = 0x1p-96;
constexpr double TWO_P64 = 0x1p+64;

template <int MODEL> struct model_dim { static constexpr int value = (MODEL == MODEL_UCSV_RB) ? 4 : (MODEL == MODEL_UCSV3D) ? 3 : 1; };
// normals a particle consumes per step (Philox slots SLOT_NORMAL0 .. SLOT_NORMAL0 + nz - 1): one per state coordinate, except
// for a marginal family, whose Kalman rows (m, P) are computed and not drawn
template <int MODEL> struct model_nz { static constexpr int value = (MODEL == MODEL_UCSV_RB) ? 2 : model_dim<MODEL>::value; };
// marginal families: the step sees y and returns the log-weight (model_marginal_step below); the first step too
template <int MODEL> struct model_marginal { static constexpr bool value = MODEL == MODEL_UCSV_RB; };
constexpr int MAX_DIM = 4;       // largest state dimension of a family

SMC_HD int model_dim_rt(int id) { return id == MODEL_UCSV_RB ? 4 : id == MODEL_UCSV3D ? 3 : (id == MODEL_LG1D || id == MODEL_SV1D) ? 1 : -1; }
SMC_HD int model_nraw_rt(int id) {
    return id == MODEL_LG1D ? 6 : id == MODEL_SV1D ? 3 : (id == MODEL_UCSV3D || id == MODEL_UCSV_RB) ? 5 : -1;
}

// ---- bit casts -------------------------------------------------------------------------
SMC_HD double bits2d(uint64_t b) { return __builtin_bit_cast(double, b); }
SMC_HD uint64_t d2bits(double d) { return __builtin_bit_cast(uint64_t, d); }
SMC_HD double pow2i(int k) { return bits2d((uint64_t)(k + 1023) << 52); }  // 2^k, k in [-1022,1023]
// v * 2^k for a result in the normal range: the same bits as v * pow2i(k) (an exact scaling either way); one v_ldexp_f64
// on the device instead of building the power of two and multiplying
SMC_HD double scale2(double v, int k) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_ldexp(v, k);
#else
    return v * pow2i(k);
#endif
}
SMC_HD double inf() { return bits2d(0x7ff0000000000000ULL); }

// round to nearest even: signed |v| < 2^51 ; non-negative of any size
SMC_HD double rne(double v) { return (v + 0x1.8p52) - 0x1.8p52; }
SMC_HD double rne_pos(double v) { return v < 0x1p52 ? (v + 0x1p52) - 0x1p52 : v; }

// ---- Philox4x32-10 ---------------------------------------------------------------------
struct u32x4 { uint32_t v[4]; };

SMC_HD uint32_t mulhi32(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}

// a ^ b ^ c: one v_bitop3_b32 on gfx950 (the compiler does not form it by itself)
SMC_HD uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
#else
    return a ^ b ^ c;
#endif
}

// a ^ (b & c): one v_bitop3_b32 as well
SMC_HD uint32_t xor_and(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x78);   // 0xF0 ^ (0xCC & 0xAA)
#else
    return a ^ (b & c);
#endif
}

SMC_HD u32x4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        // full 32x32 -> 64 products (one v_mad_u64_u32 each on the device)
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t h0 = (uint32_t)(p0 >> 32), l0 = (uint32_t)p0;
        const uint32_t h1 = (uint32_t)(p1 >> 32), l1 = (uint32_t)p1;
        const uint32_t n0 = xor3(h1, c1, k0), n2 = xor3(h0, c3, k1);
        c0 = n0; c1 = l1; c2 = n2; c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return u32x4{{c0, c1, c2, c3}};
}

SMC_HD u32x4 draw(uint64_t seed, uint32_t pair, uint32_t stream, uint32_t t, uint32_t slot) {
    return philox4x32_10(pair, stream, t, slot, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// fma(p, r, c) with a compile-time constant c.  On the device the constant sits in a scalar register pair filled by two
// s_mov_b32 (scalar issue port) and the instruction is the three-source v_fma_f64: the compiler's own choice, v_fmac_f64,
// accumulates INTO the constant and so first copies every coefficient into vector registers - two v_mov_b32 per
// coefficient, 29 % of Box-Muller's vector instructions.  Same IEEE fused multiply-add, same bits.
#if defined(__HIP_DEVICE_COMPILE__)
template <uint64_t BITS>
__device__ __forceinline__ double fma_const(double p, double r) {
    uint32_t lo, hi;
    double d;
    asm("s_mov_b32 %0, %1" : "=s"(lo) : "n"((uint32_t)BITS));
    asm("s_mov_b32 %0, %1" : "=s"(hi) : "n"((uint32_t)(BITS >> 32)));
    const double c = __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(d) : "v"(p), "v"(r), "s"(c));
    return d;
}
#define SMC_FMAK(p, r, c) fma_const<__builtin_bit_cast(uint64_t, (double)(c))>((p), (r))
#else
#define SMC_FMAK(p, r, c) fma((p), (r), (c))
#endif

// ---- division and square root without their range handling ---------------------------------
// n / d and sqrt(x) for operands of moderate magnitude: the refinement sequences of the compiler's IEEE expansions without
// the operand scaling (v_div_scale, v_ldexp) and the special-value fix-ups around them - inactive for these operands, so the
// results are the same bits (the host side, and the oracle, use the correctly rounded library operations they reproduce).
#if defined(__HIP_DEVICE_COMPILE__)
// |d| in [2^-500, 2^500], n zero or |n / d| in [2^-500, 2^500]
__device__ __forceinline__ double div_moderate(double n, double d) {
    double y = __builtin_amdgcn_rcp(d);
    double e = fma(-d, y, 1.0);
    y = fma(y, e, y);
    e = fma(-d, y, 1.0);
    y = fma(y, e, y);
    const double q = n * y;
    const double r = fma(-d, q, n);
    return fma(r, y, q);
}
// x = -0.0 or x in [2^-500, 2^500]   (sqrt(-0.0) = -0.0: the refinement turns it into NaN, which the maximum drops)
__device__ __forceinline__ double sqrt_moderate_or_negzero(double x) {
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y;
    double h = y * 0.5;
    const double r = fma(-h, g, 0.5);
    g = fma(g, r, g);
    double d = fma(-g, g, x);
    h = fma(h, r, h);
    g = fma(d, h, g);
    d = fma(-g, g, x);
    g = fma(d, h, g);
    return __builtin_fmax(g, -0.0);
}
#else
inline double div_moderate(double n, double d) { return n / d; }
inline double sqrt_moderate_or_negzero(double x) { return sqrt(x); }
#endif

// ---- exp / log / sincos ----------------------------------------------------------------
// exp(x) = p * 2^k, k = rint(x / ln2) returned as an integral double, p in [0.707, 1.415]; |x| <= 7e8
// the two halves of sp_exp_parts: k alone (two instructions), and p once k is known
SMC_HD double sp_exp_k(double x) { return rne(x * INV_LN2); }
SMC_HD double sp_exp_p(double x, double k);
SMC_HD double sp_exp_parts(double x, double& kout) {
    const double k = sp_exp_k(x);
    kout = k;
    return sp_exp_p(x, k);
}
SMC_HD double sp_exp_p(double x, double k) {
    double r = fma(-k, LN2_HI, x);
    r = fma(-k, LN2_LO, r);
    double p = 0x1.6124613a86d09p-33;
    p = SMC_FMAK(p, r, 0x1.1eed8eff8d898p-29);
    p = SMC_FMAK(p, r, 0x1.ae64567f544e4p-26);
    p = SMC_FMAK(p, r, 0x1.27e4fb7789f5cp-22);
    p = SMC_FMAK(p, r, 0x1.71de3a556c734p-19);
    p = SMC_FMAK(p, r, 0x1.a01a01a01a01ap-16);
    p = SMC_FMAK(p, r, 0x1.a01a01a01a01ap-13);
    p = SMC_FMAK(p, r, 0x1.6c16c16c16c17p-10);
    p = SMC_FMAK(p, r, 0x1.1111111111111p-7);
    p = SMC_FMAK(p, r, 0x1.5555555555555p-5);
    p = SMC_FMAK(p, r, 0x1.5555555555555p-3);
    p = SMC_FMAK(p, r, 0.5);
    p = SMC_FMAK(p, r, 1.0);
    p = SMC_FMAK(p, r, 1.0);
    return p;
}

SMC_HD double sp_exp(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    // branch-free on the device (as three nested divergent branches the calls of a thread could not overlap): the body runs on
    // whatever x is - nothing in it traps - and the two range cases are selected afterwards; a NaN passes both comparisons
    // and comes out of the arithmetic as itself
    double k;
    const double p = sp_exp_parts(x, k);
    double r = scale2(p, (int)k);    // x in (-708, 709]: a normal number
    r = x > 709.0 ? inf() : r;
    r = x <= -708.0 ? 0.0 : r;
    return r;
#else
    if (x != x) return x;
    if (!(x > -708.0)) return 0.0;
    if (x > 709.0) return inf();
    double k;
    const double p = sp_exp_parts(x, k);
    return scale2(p, (int)k);        // x > -708: the result is a normal number
#endif
}

// a log-weight takes part in the normalisation iff it is a number of sane magnitude
SMC_HD bool lw_alive(double l) { return l == l && (l < 0.0 ? -l : l) <= 7e8; }   // |k| < 2^30: differences fit int32

// q = rint(p * 2^(bits + dk)),  dk = k_i - kb <= 0 (integral doubles)
SMC_HD uint64_t fix_weight(double p, double dk, int bits) {
    if (dk < -(double)(bits + 2)) return 0;
    return (uint64_t)rne_pos(p * pow2i(bits + (int)dk));
}
// the same value for an integer exponent difference, with the rounding and the conversion done by
// ONE addition: v < 2^50, so v + 2^52 holds rint(v) in its low mantissa bits
SMC_HD uint64_t fix_weight_i(double p, int dk, int bits) {
    if (dk < -(bits + 2)) return 0;
    return d2bits(p * pow2i(bits + dk) + 0x1p52) & 0x000fffffffffffffULL;
}

// log(x) for x positive, finite and normal (no special cases to test): the body of sp_log, in the pieces the staged Box-Muller
// below runs one at a time
// x = m 2^e with m in (sqrt(1/2), sqrt(2)]; f = m - 1
SMC_HD void log_split(double x, int e0, int& e, double& f) {
    const uint64_t b = d2bits(x);
    // m in (sqrt(1/2), sqrt(2)], x = m 2^e: the mantissa bits decide (m > sqrt 2 as doubles of equal exponent), and the
    // exponent field of m is written directly (0x3fe halves it)
    const uint64_t mant = b & 0x000fffffffffffffULL;
    const bool up = mant > (0x3ff6a09e667f3bcdULL & 0x000fffffffffffffULL);
    e = e0 + (int)((b >> 52) & 0x7ff) - 1023 + (up ? 1 : 0);
    const double m = bits2d(mant | (up ? 0x3fe0000000000000ULL : 0x3ff0000000000000ULL));
    f = m - 1.0;
}
constexpr double LOG_R0 = 0x1.642c8590b2164p-4;
constexpr int LOG_NC = 10;
constexpr double LOG_C[LOG_NC] = {0x1.8618618618618p-4, 0x1.af286bca1af28p-4, 0x1.e1e1e1e1e1e1ep-4, 0x1.1111111111111p-3,
                                  0x1.3b13b13b13b14p-3, 0x1.745d1745d1746p-3, 0x1.c71c71c71c71cp-3, 0x1.2492492492492p-2,
                                  0x1.999999999999ap-2, 0x1.5555555555555p-1};
// Horner steps A .. B-1 of a polynomial with the coefficients C (compile-time constants: SMC_FMAK)
#define SMC_POLY_STEPS(name, C)                                        \
    template <int A, int B>                                            \
    SMC_HD double name(double p, double z) {                           \
        if constexpr (A < B) return name<A + 1, B>(SMC_FMAK(p, z, C[A]), z); \
        else return p;                                                 \
    }
SMC_POLY_STEPS(log_poly, LOG_C)
// log x from e, f, s = f / (2 + f) and the polynomial R(s^2) s^2
SMC_HD double log_combine(int e, double f, double s, double Rz) {
    const double dk = (double)e;
    return dk * LN2_HI - ((s * (f - Rz) - dk * LN2_LO) - f);
}
SMC_HD double sp_log_normal(double x, int e0) {
    int e;
    double f;
    log_split(x, e0, e, f);
    const double s = div_moderate(f, 2.0 + f);   // f in [-0.2929, 0.4143]: zero or of magnitude >= 2^-53
    const double z = s * s;
    const double R = log_poly<0, LOG_NC>(LOG_R0, z);
    return log_combine(e, f, s, R * z);
}

SMC_HD double sp_log(double x) {
    if (x != x || x < 0.0) return bits2d(0x7ff8000000000000ULL);
    if (x == 0.0) return -inf();
    if (x == inf()) return x;
    int e = 0;
    if (x < 0x1p-1022) { x *= 0x1p54; e = -54; }
    return sp_log_normal(x, e);
}

// cos, sin of 2*pi*u for u in [0,1) a multiple of 2^-53, in pieces as well
// the octant of u, y in [0, pi/4] and z = y^2
SMC_HD void sc_reduce(double u, int& oct, double& y, double& z) {
    const double a = 8.0 * u;
    oct = (int)a;
    // g = a - oct in the even octants, 1 - (a - oct) in the odd ones: |(oct rounded up to even) - a|, exact either way
    const double g = fabs((double)(oct + (oct & 1)) - a);
    y = g * PIO4;
    z = y * y;
}
constexpr double SIN_P0 = 0x1.952c77030ad4ap-49;
constexpr int SIN_NC = 7;
constexpr double SIN_C[SIN_NC] = {-0x1.ae7f3e733b81fp-41, 0x1.6124613a86d09p-33, -0x1.ae64567f544e4p-26, 0x1.71de3a556c734p-19,
                                  -0x1.a01a01a01a01ap-13, 0x1.1111111111111p-7, -0x1.5555555555555p-3};
constexpr double COS_P0 = -0x1.6827863b97d97p-53;
constexpr int COS_NC = 8;
constexpr double COS_C[COS_NC] = {0x1.ae7f3e733b81fp-45, -0x1.93974a8c07c9dp-37, 0x1.1eed8eff8d898p-29, -0x1.27e4fb7789f5cp-22,
                                  0x1.a01a01a01a01ap-16, -0x1.6c16c16c16c17p-10, 0x1.5555555555555p-5, -0.5};
SMC_POLY_STEPS(sin_poly, SIN_C)
SMC_POLY_STEPS(cos_poly, COS_C)
#undef SMC_POLY_STEPS
SMC_HD double sc_sin(double y, double z, double ps) { return fma(y * z, ps, y); }
SMC_HD double sc_cos(double z, double pc) { return SMC_FMAK(z, pc, 1.0); }
// (sin y, cos y) to (cos, sin) of the angle: swapped in the octants 1, 2, 5, 6, then the signs
SMC_HD void sc_place(int oct, double sy, double cy, double& c, double& s) {
    const bool swap = ((oct + 1) & 2) != 0;
    double cc = swap ? sy : cy;
    double ss = swap ? cy : sy;
    // cc = -cc in the octants 2..5, ss = -ss in 4..7: bit 2 of oct + 2 / of oct moved onto the sign bit
    const uint64_t cb = d2bits(cc), sb = d2bits(ss);
    const uint32_t ch = xor_and((uint32_t)(cb >> 32), ((uint32_t)oct << 29) + 0x40000000u, 0x80000000u);
    const uint32_t sh = xor_and((uint32_t)(sb >> 32), (uint32_t)oct << 29, 0x80000000u);
    c = bits2d(((uint64_t)ch << 32) | (uint32_t)cb);
    s = bits2d(((uint64_t)sh << 32) | (uint32_t)sb);
}
SMC_HD void sp_sincos2pi(double u, double& c, double& s) {
    int oct;
    double y, z;
    sc_reduce(u, oct, y, z);
    const double sy = sc_sin(y, z, sin_poly<0, SIN_NC>(SIN_P0, z));
    const double cy = sc_cos(z, cos_poly<0, COS_NC>(COS_P0, z));
    sc_place(oct, sy, cy, c, s);
}

// four Philox words -> (z0, z1) iid N(0,1); z0 belongs to particle 2p, z1 to 2p+1:
//     u1 = (n1 + 1) 2^-53, u2 = n2 2^-53 (n = the 53 high bits of a word pair)
//     r = sqrt(-2 log u1), (c, s) = sp_sincos2pi(u2), z0 = r c, z1 = r s
// written as BM_NSLICE straight-line slices over a small state: run in order they are the pieces of sp_log_normal,
// sqrt_moderate_or_negzero and sp_sincos2pi above, each operation once and in the order of the plain formula (the radius first,
// then the angle), so that box_muller, which runs them all, compiles to what the plain formula compiles to.  k_step runs the
// slices of its last pair one at a time under the probes of its LDS ancestor search (step_body, smc_kernels.h).
struct BmState {
    u32x4 w;                  // the Philox words (consumed by slice 0)
    double u1, u2;
    int e;                    // logarithm: exponent, f = m - 1, s = f / (2 + f), z = s^2, R
    double f, s, zl, R;
    double x;                 // -2 log u1, then r = sqrt(x)
    int oct;                  // sine and cosine: octant, y, z = y^2, the two polynomials, sin y
    double y, zs, ps, pc, sy;
    double z0, z1;            // slice 8: (cos, sin); slice 9: the normals
};
constexpr int BM_NSLICE = 10;
template <int I>
SMC_HD void bm_slice(BmState& b) {
    static_assert(I >= 0 && I < BM_NSLICE, "slice index");
    if constexpr (I == 0) {
        // n = (hi:lo) >> 11 = hi 2^21 + (lo >> 11): two exact terms whose sum is representable, so one fma gives it exactly
        // (instead of a 64-bit shift, a 64-bit add and a 64-bit conversion)
        b.u1 = fma((double)b.w.v[1], 0x1p-32, (double)((b.w.v[0] >> 11) + 1u) * TWO_M53);
        b.u2 = fma((double)b.w.v[3], 0x1p-32, (double)(b.w.v[2] >> 11) * TWO_M53);
    } else if constexpr (I == 1) {
        // u1 in [2^-53, 1] (positive, finite, normal): -2 log u1 is -0.0 (u1 = 1) or in [2.2e-16, 73.5]
        log_split(b.u1, 0, b.e, b.f);
        b.s = div_moderate(b.f, 2.0 + b.f);   // f in [-0.2929, 0.4143]: zero or of magnitude >= 2^-53
    } else if constexpr (I == 2) {
        b.zl = b.s * b.s;
        b.R = log_poly<0, 7>(LOG_R0, b.zl);
    } else if constexpr (I == 3) {
        b.R = log_poly<7, LOG_NC>(b.R, b.zl);
        b.x = -2.0 * log_combine(b.e, b.f, b.s, b.R * b.zl);
    } else if constexpr (I == 4) {
        b.x = sqrt_moderate_or_negzero(b.x);
    } else if constexpr (I == 5) {
        sc_reduce(b.u2, b.oct, b.y, b.zs);
        b.ps = sin_poly<0, 4>(SIN_P0, b.zs);
    } else if constexpr (I == 6) {
        b.ps = sin_poly<4, SIN_NC>(b.ps, b.zs);
        b.sy = sc_sin(b.y, b.zs, b.ps);
        b.pc = cos_poly<0, 2>(COS_P0, b.zs);
    } else if constexpr (I == 7) {
        b.pc = cos_poly<2, COS_NC>(b.pc, b.zs);
    } else if constexpr (I == 8) {
        sc_place(b.oct, b.sy, sc_cos(b.zs, b.pc), b.z0, b.z1);
    } else {
        b.z0 = b.x * b.z0;
        b.z1 = b.x * b.z1;
    }
}
template <int A, int B>
SMC_HD void bm_slices(BmState& b) {   // slices A .. B-1
    if constexpr (A < B) {
        bm_slice<A>(b);
        bm_slices<A + 1, B>(b);
    }
}
SMC_HD void box_muller(const u32x4& w, double& z0, double& z1) {
    BmState b;
    b.w = w;
    bm_slices<0, BM_NSLICE>(b);
    z0 = b.z0;
    z1 = b.z1;
}

// ---- 64x64 -> 128 multiply ---------------------------------------------------------------
SMC_HD void mul64wide(uint64_t a, uint64_t b, uint64_t& hi, uint64_t& lo) {
#if defined(__HIP_DEVICE_COMPILE__)
    hi = __umul64hi(a, b);
    lo = a * b;
#else
    const unsigned __int128 p = (unsigned __int128)a * b;
    hi = (uint64_t)(p >> 64);
    lo = (uint64_t)p;
#endif
}

// ---- break points of a multinomial resampling step (multi-segment filters) ------------------
// The n iid uniforms of resample() are generated sorted BY BLOCK (block = the seg consecutive children one
// workgroup owns): with E_i iid Exp(1) the order statistics are U_(k) = (E_1+..+E_k)/(E_1+..+E_{n+1}); a
// block of m ranks adds a Gamma(m) variate to these sums, so the largest uniform of block w is
// F_{w+1} = (g_0+..+g_w)/(g_0+..+g_{B-1}+e) and, given the break points, the other m-1 uniforms of the
// block are iid on (F_w, F_{w+1}).  The break points do not depend on the particles: a small kernel
// computes them for many steps ahead.  Everything after the Gamma variates is integer arithmetic.
SMC_HD double uniform53(const u32x4& w) {   // (0, 1], 53 bits, from words 0 and 1
    return (double)(((((uint64_t)w.v[1] << 32) | w.v[0]) >> 11) + 1) * TWO_M53;
}
// Gamma(m, 1), integer shape m >= 1, in 2^-32 fixed point (Marsaglia & Tsang 2000)
SMC_HD uint64_t gamma_fix(uint64_t seed, uint32_t w, uint32_t stream, uint32_t t, int64_t m) {
    const double d = (double)m - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
    double G = d;   // (all 8 attempts rejected: probability ~1e-15)
    for (uint32_t it = 0; it < 8; ++it) {
        double x, z1;
        box_muller(draw(seed, w, stream, t, SLOT_BREAK + 2 * it), x, z1);
        const double vv = 1.0 + c * x;
        if (!(vv > 0.0)) continue;
        const double v3 = vv * vv * vv, x2 = x * x;
        const double u = uniform53(draw(seed, w, stream, t, SLOT_BREAK + 2 * it + 1));
        if (u < 1.0 - 0.0331 * (x2 * x2) || sp_log(u) < 0.5 * x2 + d * ((1.0 - v3) + sp_log(v3))) {
            G = d * v3;
            break;
        }
    }
    const uint64_t g = (uint64_t)rne_pos(G * 0x1p32);
    return g ? g : 1;
}
SMC_HD uint64_t exp1_fix(uint64_t seed, uint32_t w, uint32_t stream, uint32_t t) {   // Exp(1), 2^-32 fixed point, >= 1 ulp
    const uint64_t e = (uint64_t)rne_pos(-sp_log(uniform53(draw(seed, w, stream, t, SLOT_BREAK + 1))) * 0x1p32);
    return e ? e : 1;
}
// floor(P * 2^64 / S) for P < S < 2^63 (binary long division: used once per block and step, off the hot path)
SMC_HD uint64_t div_frac64(uint64_t P, uint64_t S) {
    uint64_t rem = P, q = 0;
    for (int i = 0; i < 64; ++i) {
        rem <<= 1;
        q <<= 1;
        if (rem >= S) { rem -= S; q |= 1; }
    }
    return q;
}

// ---- systematic resampling targets (opt-in; SMC_FLAG_SYSTEMATIC) ---------------------------
// exact q = floor(D / N), r = D mod N for D < 2^63, 1 <= N < 2^31, without an integer divider:
// double-precision estimates through inv = 1/N (the first off by at most 2^12, the second by at most 1)
// followed by an exact integer correction of the remainder - the result is exact by construction.
SMC_HD void divmod_u64_u32(uint64_t D, uint32_t N, double inv, uint64_t& q, uint32_t& r) {
    if ((N & (N - 1u)) == 0u) {   // power of two: the common particle counts
        const int sft = __builtin_ctz(N);
        q = D >> sft;
        r = (uint32_t)(D & (uint64_t)(N - 1u));
        return;
    }
    uint64_t q1 = (uint64_t)((double)D * inv);
    int64_t r1 = (int64_t)(D - q1 * (uint64_t)N);          // |r1| < 2^44: exact in a double
    const int64_t q2 = (int64_t)floor((double)r1 * inv);
    q1 += (uint64_t)q2;
    r1 -= q2 * (int64_t)N;
    if (r1 < 0) { q1 -= 1; r1 += N; }
    if (r1 >= (int64_t)N) { q1 += 1; r1 -= N; }
    q = q1;
    r = (uint32_t)r1;
}
// T_j = floor((j * Dtot + v0) / n), v0 = mulhi64(u, Dtot), for the children j = j0 + k, k < 2^13:
// with Dtot = dq n + dr, v0 = q0 n + r0 and r0 + j0 dr = qa n + ra,
//     T_j = (q0 + j0 dq + qa) + k dq + floor((ra + k dr) / n),   ra + k dr < 2^44.
struct SysBase {
    uint64_t Tbase, dq;
    double inv;
    uint32_t ra, dr, n;
};
// inv = 1.0 / (double)n (a per-filter constant: the host passes it in)
SMC_HD SysBase sys_base(uint64_t Dtot, uint32_t n, double inv, uint64_t u, uint64_t j0) {
    uint64_t v0, lo;
    mul64wide(u, Dtot, v0, lo);
    SysBase sb;
    sb.n = n;
    sb.inv = inv;
    uint64_t q0, qa;
    uint32_t r0;
    divmod_u64_u32(Dtot, n, sb.inv, sb.dq, sb.dr);
    divmod_u64_u32(v0, n, sb.inv, q0, r0);
    divmod_u64_u32((uint64_t)r0 + j0 * (uint64_t)sb.dr, n, sb.inv, qa, sb.ra);
    sb.Tbase = q0 + j0 * sb.dq + qa;
    return sb;
}
SMC_HD uint64_t sys_target(const SysBase& sb, uint32_t k) {
    const uint64_t e = (uint64_t)sb.ra + (uint64_t)k * sb.dr;   // < 2^44
    uint64_t qe;
    if ((sb.n & (sb.n - 1u)) == 0u) {
        qe = e >> __builtin_ctz(sb.n);
    } else {
        qe = (uint64_t)((double)e * sb.inv);                    // floor(e / n) or one off: settle it exactly
        const int64_t rem = (int64_t)(e - qe * (uint64_t)sb.n);
        qe = rem < 0 ? qe - 1 : (rem >= (int64_t)sb.n ? qe + 1 : qe);
    }
    return sb.Tbase + (uint64_t)k * sb.dq + qe;
}
// (C >> sh) > T2  <=>  C > sys_threshold(T2, sh)
SMC_HD uint64_t sys_threshold(uint64_t T2, int sh) { return sh < 64 ? ((T2 + 1) << sh) - 1 : 0; }

SMC_HD double u128_to_double(uint64_t hi, uint64_t lo) { return (double)hi * TWO_P64 + (double)lo; }

SMC_HD int ceil_log2_i64(int64_t n) {
    int k = 0;
    while (((int64_t)1 << k) < n) ++k;
    return k;
}

// ---- models ------------------------------------------------------------------------------
// raw rows:  LG1D (A,B,Q,R,x0,sigma0)  Q,R,sigma0 VARIANCES (ssm.jl:93,102,108)
//            SV1D (mu,rho,sigma)
//            UCSV (gamma_eps,gamma_eta,x0,lse0,lsn0)  gammas STD-DEVs (ssm.jl:239-240); UCSV_RB: the same row
// der rows:  LG1D (sQ,sR,s0,1/sR,c_obs)   SV1D (s0)
struct Params {
    double raw[NPARAM];
    double der[NPARAM];
};
// the proposal of a guided filter ("proposals" below), a table of its own beside the parameter rows: bootstrap handles have none
//            LG1D (c0,c1,c2,s2, ss,1/ss,1/sQ,log ss - log sQ)
struct PropRow {
    double p[NPARAM];
};

SMC_HD void derive_params(int model, const double* raw, double* der) {
    for (int k = 0; k < NPARAM; ++k) der[k] = 0.0;
    if (model == MODEL_LG1D) {
        const double sR = sqrt(raw[3]);
        der[0] = sqrt(raw[2]);
        der[1] = sR;
        der[2] = sqrt(raw[5]);
        der[3] = 1.0 / sR;
        der[4] = -HALF_LOG2PI - sp_log(sR);
    } else if (model == MODEL_SV1D) {
        der[0] = raw[2] / sqrt(1.0 - raw[1] * raw[1]);
    }
}

// x = rand(initial_dist(model))            ssm.jl:105-109, 249-259
template <int MODEL>
SMC_HD void model_initial(const Params& p, const double* z, double* x) {
    if constexpr (MODEL == MODEL_LG1D) {
        x[0] = fma(p.der[2], z[0], p.raw[4]);
    } else if constexpr (MODEL == MODEL_SV1D) {
        x[0] = fma(p.der[0], z[0], p.raw[0]);
    } else {
        x[0] = fma(sp_exp(0.5 * p.raw[3]), z[0], p.raw[2]);
        x[1] = fma(p.raw[0], z[1], p.raw[3]);
        x[2] = fma(p.raw[1], z[2], p.raw[4]);
    }
}

// x = rand(transition(model, xp))          ssm.jl:87-94, 233-242
template <int MODEL>
SMC_HD void model_transition(const Params& p, const double* xp, const double* z, double* x) {
    if constexpr (MODEL == MODEL_LG1D) {
        x[0] = fma(p.der[0], z[0], p.raw[0] * xp[0]);
    } else if constexpr (MODEL == MODEL_SV1D) {
        x[0] = fma(p.raw[2], z[0], fma(p.raw[1], xp[0] - p.raw[0], p.raw[0]));
    } else {
        x[0] = fma(sp_exp(0.5 * xp[1]), z[0], xp[0]);
        x[1] = fma(p.raw[0], z[1], xp[1]);
        x[2] = fma(p.raw[1], z[2], xp[2]);
    }
}

// logpdf(observation(model, x), y)          ssm.jl:96-103, 244-247
template <int MODEL>
SMC_HD double model_logobs(const Params& p, const double* x, double y) {
    double z, c;
    if constexpr (MODEL == MODEL_LG1D) {
        z = (y - p.raw[1] * x[0]) * p.der[3];
        c = p.der[4];
    } else if constexpr (MODEL == MODEL_SV1D) {
        z = y * sp_exp(-0.5 * x[0]);
        c = fma(-0.5, x[0], -HALF_LOG2PI);
    } else {
        z = (y - x[0]) * sp_exp(-0.5 * x[2]);
        c = fma(-0.5, x[2], -HALF_LOG2PI);
    }
    return fma(-0.5 * z, z, c);
}

template <int MODEL>
SMC_HD void model_obs_moments(const Params& p, const double* x, double& mean, double& sd) {
    if constexpr (MODEL == MODEL_LG1D) {
        mean = p.raw[1] * x[0];
        sd = p.der[1];
    } else if constexpr (MODEL == MODEL_SV1D) {
        mean = 0.0;
        sd = sp_exp(0.5 * x[0]);
    } else {
        mean = x[0];
        sd = sp_exp(0.5 * x[2]);
    }
}

// ---- proposals: the guided particle filter (particle_filter / particle_filter!, particles.jl:28-84) ------------------------
// Every step after the first draws x from proposal(xp, y) instead of the transition and weights it by (particles.jl:72-80)
//     logw = logpdf(observation(x), y) + logpdf(transition(xp), x) - logpdf(proposal(xp, y), x).
// The proposals are enumerated like the model families.  A guided step consumes the normals of the bootstrap step: one per
// state coordinate, the same Philox slots.
//   PROP_AFFINE  (LG1D)  row (c0, c1, c2, s2), s2 a variance:  m = c0 + c1 xp + c2 y,  x = m + sqrt(s2) z
//   PROP_OPTIMAL (LG1D)  the AFFINE row derived from the model row: D = B B Q + R, (0, A R / D, B Q / D, Q R / D)
//   PROP_OPTIMAL (UCSV)  the log-volatilities move by the transition (same normals); with Q = exp(xp[1]), R = exp(x[2]),
//                        K = Q / (Q + R):  x[0] = xp[0] + K (y - xp[0]) + sqrt(K R) z[0],  logw = logN(y; xp[0], Q + R)
//                        (the three terms collapse to this closed form; it does not depend on x[0])
// Order of operations of the LG1D step (model_guided): k = fma(c2, y, c0), replaced by -0.0 when it is zero, so that
// m = fma(c1, xp, k) is then the rounded product c1 xp with its sign of zero; x = fma(ss, z, m);
//     zt = (x - A xp) / sQ, zp = (x - m) / ss (as products with the stored reciprocals),
//     logw = logobs(x, y) + (((0.5 zp) zp - (0.5 zt) zt) + (log ss - log sQ)).
// With the row (0, A, 0, Q) every operand of the bracket coincides, it evaluates to +0.0, and the step is the bootstrap step
// bit for bit.  The FIRST step of a guided filter is the bootstrap first step (initial_dist, observation weight): the reference
// adds logpdf(initial_dist, x) there (particles.jl:41-44), a slip - its own commented line :43 shows the intended correction,
// which is zero for a draw from initial_dist.
constexpr int PROP_NONE = 0;
constexpr int PROP_AFFINE = 1;
constexpr int PROP_OPTIMAL = 2;
constexpr int PROP_NPAR = 4;

SMC_HD bool proposal_supported(int model, int kind) {
    return kind == PROP_NONE || (model == MODEL_LG1D && (kind == PROP_AFFINE || kind == PROP_OPTIMAL)) ||
           (model == MODEL_UCSV3D && kind == PROP_OPTIMAL);
}
// the locally optimal proposal of an LG1D row as an AFFINE row.  Each entry is a quotient of a product by D = B B Q + R; D and the
// products are carried with their rounding errors (fma residuals, a two-sum) and the quotient gets one correction step, so
// every entry is within one ulp of the formula whatever the row (a plain evaluation rounds five times).  Once per filter.
SMC_HD double quotient_corrected(double a, double b, double D, double De) {   // (a b) / (D + De)
    const double n = a * b, ne = fma(a, b, -n);
    const double c = n / D;
    const double r = fma(-c, D, n);
    return c + ((r + ne) - c * De) / D;
}
SMC_HD void optimal_proposal_lg(const double* raw, double* par) {
    const double A = raw[0], B = raw[1], Q = raw[2], R = raw[3];
    const double p = B * B, pe = fma(B, B, -p);
    const double q = p * Q, qe = fma(p, Q, -q) + pe * Q;
    const double D = q + R, t = D - q;
    const double De = ((q - (D - t)) + (R - t)) + qe;
    par[0] = 0.0;
    par[1] = quotient_corrected(A, R, D, De);
    par[2] = quotient_corrected(B, Q, D, De);
    par[3] = quotient_corrected(Q, R, D, De);
}
// the proposal row of a parameter row: OPTIMAL fills the four parameters from raw, AFFINE keeps the ones in prop[0..3]; then
// the constants of the step.  der = derive_params(raw).  PROP_NONE and UCSV (nothing to store): zeros.
SMC_HD void derive_proposal(int model, int kind, const double* raw, const double* der, double* prop) {
    if (model != MODEL_LG1D || kind == PROP_NONE) {
        for (int k = 0; k < NPARAM; ++k) prop[k] = 0.0;
        return;
    }
    if (kind == PROP_OPTIMAL) optimal_proposal_lg(raw, prop);
    const double ss = sqrt(prop[3]);
    prop[4] = ss;
    prop[5] = 1.0 / ss;
    prop[6] = 1.0 / der[0];
    prop[7] = sp_log(ss) - sp_log(der[0]);
}

// x = rand(proposal(model, xp, y)); returns the log-weight of the guided step (LG1D: AFFINE rows, UCSV: OPTIMAL)
template <int MODEL>
SMC_HD double model_guided(const Params& p, const PropRow& q, const double* xp, const double* z, double y, double* x) {
    if constexpr (MODEL == MODEL_LG1D) {
        const double k = fma(q.p[2], y, q.p[0]);
        const double m = fma(q.p[1], xp[0], k == 0.0 ? -0.0 : k);
        x[0] = fma(q.p[4], z[0], m);
        const double zt = (x[0] - p.raw[0] * xp[0]) * q.p[6];
        const double zp = (x[0] - m) * q.p[5];
        return model_logobs<MODEL>(p, x, y) + (((0.5 * zp) * zp - (0.5 * zt) * zt) + q.p[7]);
    } else if constexpr (MODEL == MODEL_UCSV3D) {
        x[1] = fma(p.raw[0], z[1], xp[1]);
        x[2] = fma(p.raw[1], z[2], xp[2]);
        const double Q = sp_exp(xp[1]), R = sp_exp(x[2]);
        const double D = Q + R, iD = 1.0 / D, K = Q * iD, e = y - xp[0];
        x[0] = fma(sqrt(K * R), z[0], fma(K, e, xp[0]));
        return fma(-0.5 * (e * iD), e, fma(-0.5, sp_log(D), -HALF_LOG2PI));
    } else {
        x[0] = xp[0] + z[0] * y;   // (no proposal for this family: never instantiated by the library)
        return bits2d(0x7ff8000000000000ULL);
    }
}

// ---- marginal families: the Rao-Blackwellised UCSV filter (MODEL_UCSV_RB) -------------------------------------------------
// Given the two log-volatility paths of UCSV (ssm.jl:215-263) the pair (x, y) is linear-Gaussian with A = B = 1, so the trend
// x is integrated out exactly by the scalar Kalman recursion (kalman_filter.jl:29-53) carried inside each particle.  State rows
// (m, lse, lsn, P): rows 1, 2 are UCSV's log-volatilities, row 0 the filtered MEAN of the trend, row 3 its filtered VARIANCE -
// always the posterior after the step's y.  The parameter row is UCSV's, with the reference's conventions: x moves with the
// PREVIOUS lse, the gammas are standard deviations, x_1 ~ N(x0, exp(lse0 / 2)).
// One step, given y (sp = the ancestor's state; `first`: t = 1, where sp is not read):
//     (m, a, b, P-) = first ? (x0, lse0, lsn0, Q) : (sp[0], sp[1], sp[2], sp[3] + Q),   Q = sp_exp(a)
//     s[1] = fma(g_eps, z[0], a);  s[2] = fma(g_eta, z[1], b)                           (UCSV's transition of the volatilities)
//     R = sp_exp(s[2]);  S = P- + R;  iS = 1 / S;  e = y - m;  K = P- iS
//     s[0] = fma(K, e, m);  s[3] = min(K R, P-)
//     logw = fma(-0.5 (e iS), e, fma(-0.5, sp_log(S), -HALF_LOG2PI))                   (log N(y; m, S), as the guided UCSV step)
// P' = P- R / S in PRODUCT form (never P- - K P-, which cancels and can turn negative): K <= 1 and R iS <= 1 as rounded values,
// so 0 < P' <= R; the minimum with P- removes the last-place excess the two roundings of K R can leave when R >> P-.
// Normals: TWO per particle and step, z[0] for lse (Philox slot SLOT_NORMAL0) and z[1] for lsn (slot SLOT_NORMAL0 + 1), each slot
// a Box-Muller pair shared by the particles 2p, 2p + 1 like every state normal - one Philox call and one Box-Muller per particle
// and step, none discarded.  (Bootstrap UCSV draws three: slots 1, 2, 3 = x, lse, lsn.)
// model_obs_moments is UCSV's (mean = row 0, sd = exp(row 2 / 2)): the observation given the filtered mean.  No proposals.
template <int MODEL>
SMC_HD double model_marginal_step(const Params& p, bool first, const double* sp, const double* z, double y, double* s) {
    static_assert(MODEL == MODEL_UCSV_RB, "marginal families");
    const double m = first ? p.raw[2] : sp[0];
    const double a = first ? p.raw[3] : sp[1];
    const double b = first ? p.raw[4] : sp[2];
    const double Q = sp_exp(a);
    const double Pm = first ? Q : sp[3] + Q;
    s[1] = fma(p.raw[0], z[0], a);
    s[2] = fma(p.raw[1], z[1], b);
    const double R = sp_exp(s[2]);
    const double S = Pm + R, iS = 1.0 / S, e = y - m;
    const double K = Pm * iS, KR = K * R;
    s[0] = fma(K, e, m);
    s[3] = KR < Pm ? KR : Pm;
    return fma(-0.5 * (e * iS), e, fma(-0.5, sp_log(S), -HALF_LOG2PI));
}

// ---- forecasts: the cloud propagated past the last observation -----------------------------------------------------------------
// p(x_{T+k} | y_1:T) and p(y_{T+k} | y_1:T), k = 1..H, from the filtered cloud (x_T, w_T).  Without an observation there is
// nothing to weigh: no resampling, no normalisation - every particle is a chain of its own that moves by the TRANSITION law
// (a guided handle too: a proposal has no role without y) and keeps the weight it has.  One forecast step of one particle:
//   bootstrap families   x_k = model_transition(x_{k-1}, z);  (ym, sd) = model_obs_moments(x_k);  yv = sd sd;  yf = fma(sd, e, ym)
//   MODEL_UCSV_RB        model_marginal_step with the measurement update left out.  With (m, a, b, P) = x_{k-1}:
//                        P- = P + sp_exp(a);  lse = fma(g_eps, z[0], a);  lsn = fma(g_eta, z[1], b);  x_k = (m, lse, lsn, P-);
//                        ym = m;  yv = P- + sp_exp(lsn);  yf = fma(sqrt(yv), e, ym)
// (ym, yv): mean and variance of y_{T+k} given the particle (Rao-Blackwellised over the observation noise); yf: one draw of it.
// Normals: particle i of filter m at horizon k (1-based) takes element i & 1 of
//     box_muller(draw(forecast_seed, i >> 1, stream[m], k, SLOT_NORMAL0 + c))      for the state normal c < model_nz
// and the same element of slot SLOT_OBS for e - the pair convention of the filter's own steps, under a seed of the caller's.  So
// trajectory i is a function of (parameter row, x_T[i], forecast_seed, stream, i) alone: not of H, of the launch geometry or of
// how the horizons are blocked.
template <int MODEL>
SMC_HD void model_marginal_predict(const Params& p, const double* sp, const double* z, double* s, double& ym, double& yv) {
    static_assert(MODEL == MODEL_UCSV_RB, "marginal families");
    const double m = sp[0], a = sp[1], b = sp[2];
    const double Pm = sp[3] + sp_exp(a);
    s[0] = m;
    s[1] = fma(p.raw[0], z[0], a);
    s[2] = fma(p.raw[1], z[1], b);
    s[3] = Pm;
    ym = m;
    yv = Pm + sp_exp(s[2]);
}
// x (not aliasing xp) = the state one horizon on; (yf, ym, yv) its observation rows
template <int MODEL>
SMC_HD void model_forecast_step(const Params& p, const double* xp, const double* z, double e, double* x, double& yf, double& ym, double& yv) {
    if constexpr (model_marginal<MODEL>::value) {
        model_marginal_predict<MODEL>(p, xp, z, x, ym, yv);
        yf = fma(sqrt(yv), e, ym);
    } else {
        double sd;
        model_transition<MODEL>(p, xp, z, x);
        model_obs_moments<MODEL>(p, x, ym, sd);
        yv = sd * sd;
        yf = fma(sd, e, ym);
    }
}

// ---- missing observations (opt-in per handle: SMC_FLAG_NAN_MISSING) ---------------------------------------------------------
// With the flag, a step whose observation is NaN is a MISSING step (+-inf still kill the step; without the flag a NaN kills it
// too).  It is the ordinary step with the observation's part left out: the resampling from the current weights (either resampler,
// the same Philox slots), the ancestors, the state normals of (seed, stream, t, SLOT_NORMAL0 + c) in the pair convention, the
// masking of a ragged last segment, the segment normalisation, the records and the emission are the ordinary step's, and the time
// index advances by one.  Per particle:
//   bootstrap families     x = model_transition(xp, z), or model_initial(z) at the first step
//   guided handles         the same: a proposal has no role without y (as in the forecasts)
//   MODEL_UCSV_RB          rows 1, 2 as in model_marginal_step; row 0 = m unchanged (x0 at the first step); row 3 = P- =
//                          sp[3] + sp_exp(sp[1]) (sp_exp(lse0) at the first step): model_marginal_predict without its observation
//                          rows - rows 0 and 3 are then the PREDICTIVE moments of the trend, not a posterior
// and the log-weight is +0.0.  The normalisation of n log-weights +0.0 gives logmu = +0.0, ess = n and w = 1/n exactly, so a
// missing step adds nothing to logZ, bit for bit.  A filter that is collapsed when it meets a gap takes identity ancestors (as at
// every step) and leaves the gap with uniform weights; its logZ stays -inf, because it is a running sum.
// x may alias xp.
template <int MODEL>
SMC_HD void model_missing_step(const Params& p, bool first, const double* xp, const double* z, double* x) {
    if constexpr (model_marginal<MODEL>::value) {
        const double m = first ? p.raw[2] : xp[0];
        const double a = first ? p.raw[3] : xp[1];
        const double b = first ? p.raw[4] : xp[2];
        const double Q = sp_exp(a);
        const double Pm = first ? Q : xp[3] + Q;
        x[0] = m;
        x[1] = fma(p.raw[0], z[0], a);
        x[2] = fma(p.raw[1], z[1], b);
        x[3] = Pm;
    } else {
        if (first) model_initial<MODEL>(p, z, x);
        else model_transition<MODEL>(p, xp, z, x);
    }
}

// ---- PMMH rejuvenation of the samplers (src/smc_samplers.jl:103-146), one parameter particle ------------------
// Random numbers are counter based like everything else: key = the move's seed, stream = GLOBAL index of the
// parameter particle (so results do not depend on how theta is sharded), t = chain position.
constexpr int PRIOR_UNIFORM = 1;      // par = (lo, hi)
constexpr int PRIOR_NORMAL = 2;       // par = (mu, sigma)
constexpr int PRIOR_TRUNCNORMAL = 3;  // par = (mu, sigma, lo, hi, log(Phi((hi-mu)/sigma) - Phi((lo-mu)/sigma)))
constexpr int PRIOR_LOGNORMAL = 4;    // par = (mu, sigma) of log x
constexpr int PRIOR_NPAR = 5;
struct PmmhSpec {
    int d;                              // parameter dimension
    int family[MAX_DTHETA];             // product_distribution([...]) component by component
    double par[MAX_DTHETA][PRIOR_NPAR];
    int nraw;                           // smc.model(theta): raw[k] = raw_from[k] >= 0 ? theta[raw_from[k]] : raw_const[k]
    int raw_from[NPARAM];
    double raw_const[NPARAM];
};
SMC_HD bool finite_d(double x) { return x == x && x != inf() && x != -inf(); }
// insupport(prior_i, x)   (smc_samplers.jl:116; Distributions' closed intervals)
SMC_HD bool prior_insupport(int fam, const double* par, double x) {
    switch (fam) {
    case PRIOR_UNIFORM: return par[0] <= x && x <= par[1];
    case PRIOR_NORMAL: return finite_d(x);
    case PRIOR_TRUNCNORMAL: return par[2] <= x && x <= par[3];
    case PRIOR_LOGNORMAL: return x > 0.0 && finite_d(x);
    }
    return false;
}
// logpdf(prior_i, x) for x in the support   (smc_samplers.jl:123; Normal: -(z^2 + log 2pi)/2 - log sigma)
SMC_HD double prior_logpdf(int fam, const double* par, double x) {
    switch (fam) {
    case PRIOR_UNIFORM: return -sp_log(par[1] - par[0]);
    case PRIOR_NORMAL: {
        const double z = (x - par[0]) / par[1];
        return -0.5 * (z * z + 2.0 * HALF_LOG2PI) - sp_log(par[1]);
    }
    case PRIOR_TRUNCNORMAL: {
        const double z = (x - par[0]) / par[1];
        return (-0.5 * (z * z + 2.0 * HALF_LOG2PI) - sp_log(par[1])) - par[4];
    }
    case PRIOR_LOGNORMAL: {
        const double lx = sp_log(x), z = (lx - par[0]) / par[1];
        return (-0.5 * (z * z + 2.0 * HALF_LOG2PI) - sp_log(par[1])) - lx;
    }
    }
    return -inf();
}
// insupport / logpdf of the product prior: components in order, sum from 0.0 left to right
// (D > 0: the dimension as a compile-time constant - s.d == D - so that theta stays in a kernel's registers; D = 0, the default:
//  s.d.  The loops run to MAX_DTHETA under a guard and are unrolled: every array index is a constant either way, and the
//  operations and their order are the same.)
template <int D = 0>
SMC_HD bool pmmh_insupport(const PmmhSpec& s, const double* th) {
    const int d = D > 0 ? D : s.d;
    bool ok = true;
#pragma unroll
    for (int i = 0; i < MAX_DTHETA; ++i)
        if (i < d) ok = ok && prior_insupport(s.family[i], s.par[i], th[i]);
    return ok;
}
template <int D = 0>
SMC_HD double pmmh_logprior(const PmmhSpec& s, const double* th) {
    const int d = D > 0 ? D : s.d;
    double lp = 0.0;
#pragma unroll
    for (int i = 0; i < MAX_DTHETA; ++i)
        if (i < d) lp = lp + prior_logpdf(s.family[i], s.par[i], th[i]);
    return lp;
}
// theta' = rand(MvNormal(theta, scale * Sigma)), Sigma = L L'  (smc_samplers.jl:99-100,114):
// theta'_i = theta_i + sq * sum_{k<=i} L[i][k] z_k, sq = sqrt(scale), the sum taken left to right
template <int D = 0>
SMC_HD void pmmh_propose(const PmmhSpec& s, uint64_t seed, uint32_t stream, uint32_t c, const double* th, const double* L /*[d][d]*/,
                         double sq, double* prop) {
    const int d = D > 0 ? D : s.d;
    double z[MAX_DTHETA + 1];
#pragma unroll
    for (int k = 0; k < MAX_DTHETA; k += 2)
        if (k < d) box_muller(draw(seed, (uint32_t)(k >> 1), stream, c, SLOT_PMMH_Z), z[k], z[k + 1]);
#pragma unroll
    for (int i = 0; i < MAX_DTHETA; ++i)
        if (i < d) {
            double a = 0.0;
#pragma unroll
            for (int k = 0; k <= i; ++k) a = a + L[i * d + k] * z[k];
            prop[i] = th[i] + sq * a;
        }
}
// log(rand()) of the accept test (smc_samplers.jl:129): u in (0, 1]
SMC_HD double pmmh_log_uniform(uint64_t seed, uint32_t stream, uint32_t c) {
    return sp_log(uniform53(draw(seed, 0u, stream, c, SLOT_PMMH_U)));
}
// smc.model(theta): parameter row of the model family
SMC_HD void pmmh_raw_row(const PmmhSpec& s, const double* th, double* raw /*[NPARAM]*/) {
    for (int k = 0; k < NPARAM; ++k) raw[k] = k < s.nraw ? (s.raw_from[k] >= 0 ? th[s.raw_from[k]] : s.raw_const[k]) : 0.0;
}

// ---- the exact scalar Kalman filter (src/kalman_filter.jl:29-53), one step ---------------------------------------
// kalman_filter(model, x, Sigma, y) for the univariate LinearModel row (A, B, Q, R): the prediction (:39-40; `predict` false
// leaves it out: the first step of a filter that starts at x_1 ~ N(x0, sigma0) like bootstrap_filter), the update (:43-49)
// and the step's log-likelihood (:51).  (x, S) are advanced in place.  The one definition behind smc_kalman_log_likelihood
// and the IBIS sampler (src/ibis.jl:136-140,172-177): logZ of a series is the sum of these values in step order.
SMC_HD double kalman_step(double A, double B, double Q, double R, bool predict, double y, double& x, double& S) {
    if (predict) { x = A * x; S = (A * A) * S + Q; }
    const double s = (B * B) * S + R, dy = y - B * x;
    const double K = S * B, inv = 1.0 / s;
    x = x + (K * inv) * dy;
    S = S - (K * K) * inv;
    return -0.5 * (0x1.d67f1c864beb5p+0 + sp_log(s) + (dy / s) * dy);
}
// The MISSING Kalman step (opt-in: SMC_FLAG_NAN_MISSING on an IBIS handle, `flags` of the calls without one): kalman_step with the
// observation's part left out.  The prediction is kalman_step's, the same expressions in the same association; there is no
// update; the step's value is +0.0, so logZ and logw gain +0.0 and a finite value keeps its bits.  With `predict` false (the first
// step of a filter with predict_first = 0) the state stays (x0, sigma0).  Consequences: logw is unchanged, so the ESS record of a
// missing step is the previous step's; the filtered record (xf_t, Sf_t) at a gap is the predictive pair, over which rts_gain /
// rts_back / rts_path_* run as they are (the backward pass interpolates through the gap); ibis_obs_moments at ahead = 0 gives the
// predictive law of the unobserved y_t.
SMC_HD double kalman_step_missing(double A, double Q, bool predict, double& x, double& S) {
    if (predict) { x = A * x; S = (A * A) * S + Q; }
    return 0.0;
}
// One step of a series under the flag: only a NaN y is missing (+-inf takes the ordinary step).  MISS = false is kalman_step.
template <bool MISS>
SMC_HD double kalman_step_gaps(double A, double B, double Q, double R, bool predict, double y, double& x, double& S) {
    if (MISS && y != y) return kalman_step_missing(A, Q, predict, x, S);
    return kalman_step(A, B, Q, R, predict, y, x, S);
}

// ---- the exact Kalman filter of a TWO-STATE linear model with a scalar observation (src/kalman_filter.jl:3-27, d = 2) ---------
// The models of MultivariateLinearGaussian / hodrick_prescott (state_space_models.jl:137-202) with a 2 x 2 transition:
//   x_t ~ N(A x_{t-1}, Q),  y_t ~ N(B x_t, R),  x_1 ~ N(x0, Sigma0)
// as a row of LG2_NRAW = 15 doubles
//   (A11,A12,A21,A22, B1,B2, Q11,Q21,Q22, R, x01,x02, S11,S21,S22)
// Q and Sigma0 are symmetric, stored as their lower triangle, and may be singular (hodrick_prescott: Q = [1/lambda 0; 0 0]).
// The row's id is MODEL_LG2D: a row of the exact-Kalman side only.  It is no particle-filter family (a singular Q has no
// transition density): smc_create, smc_simulate and every model table refuse it.
// One step, every product of two sums written as fma(a, b, c * d) with the SECOND term of the sum in the fma:
//   predict (left out when `predict` is false: the first step of a filter that starts at x_1 ~ N(x0, Sigma0)):
//     x- = A x;  M = A Sigma (four entries);  P = M A' + Q, its lower triangle (P11, P21, P22)
//   k = P B' (two entries);  s = B k + R;  e = y - B x-;  inv = 1 / s (the step's ONE division);  g = k inv
//   x = x- + g e;  Sigma = P - k g' (lower triangle);  value = -1/2 (log 2 pi + log s + (e inv) e)
// A covariance is carried as its lower triangle, so it is symmetric by construction.  s that is not a positive finite number
// does what kalman_step does with it: sp_log and the division make the value and the state NaN or infinite, logZ is poisoned from
// there on, nothing is tested and nothing faults.
constexpr int MODEL_LG2D = 16;
constexpr int LG2_NRAW = 15;
enum { LG2_A11 = 0, LG2_A12, LG2_A21, LG2_A22, LG2_B1, LG2_B2, LG2_Q11, LG2_Q21, LG2_Q22, LG2_R, LG2_X1, LG2_X2, LG2_S11, LG2_S21, LG2_S22 };
// x <- A x, M = A S, P = M A' + Q: the prediction, shared by the filter's step and the backward recursion
SMC_HD void kalman2_predict(const double* r, double& x1, double& x2, double S11, double S21, double S22, double* M /*[4]*/, double& P11,
                            double& P21, double& P22) {
    const double A11 = r[LG2_A11], A12 = r[LG2_A12], A21 = r[LG2_A21], A22 = r[LG2_A22];
    const double p1 = fma(A12, x2, A11 * x1), p2 = fma(A22, x2, A21 * x1);
    x1 = p1; x2 = p2;
    M[0] = fma(A12, S21, A11 * S11); M[1] = fma(A12, S22, A11 * S21);
    M[2] = fma(A22, S21, A21 * S11); M[3] = fma(A22, S22, A21 * S21);
    P11 = fma(M[1], A12, M[0] * A11) + r[LG2_Q11];
    P21 = fma(M[3], A12, M[2] * A11) + r[LG2_Q21];
    P22 = fma(M[3], A22, M[2] * A21) + r[LG2_Q22];
}
SMC_HD double kalman2_step(const double* r /*[LG2_NRAW], entries 0..9 are read*/, bool predict, double y, double& x1, double& x2, double& S11,
                           double& S21, double& S22) {
    double P11 = S11, P21 = S21, P22 = S22;
    if (predict) { double M[4]; kalman2_predict(r, x1, x2, S11, S21, S22, M, P11, P21, P22); }
    const double B1 = r[LG2_B1], B2 = r[LG2_B2];
    const double k1 = fma(P21, B2, P11 * B1), k2 = fma(P22, B2, P21 * B1);
    const double s = fma(B2, k2, B1 * k1) + r[LG2_R], e = y - fma(B2, x2, B1 * x1);
    const double inv = 1.0 / s, g1 = k1 * inv, g2 = k2 * inv;
    x1 = fma(g1, e, x1);
    x2 = fma(g2, e, x2);
    S11 = fma(-k1, g1, P11);
    S21 = fma(-k2, g1, P21);
    S22 = fma(-k2, g2, P22);
    return -0.5 * (0x1.d67f1c864beb5p+0 + sp_log(s) + (e * inv) * e);
}
// The RTS backward recursion over the filtered record (xf_t, Sf_t) of kalman2_step: (xs, Ps) of step t+1 in, of step t out.
//   x-, M, P = kalman2_predict(xf_t, Sf_t)        the prediction of step t+1, as the filter formed it
//   det = P11 P22 - P21 P21;  G = Sf_t A' P^-1 = M' adj(P) / det        (adjugate and determinant, ONE division)
//   xs_t = xf_t + G (xs_{t+1} - x-)
//   Ps_t = Sf_t + (G D) G',  D = Ps_{t+1} - P      lower triangle only: symmetric by construction
// RULE for a predicted covariance that cannot be inverted - det <= 0, or det not finite: there is no smoothed state; xs_t and
// Ps_t are NaN, and so is everything before t (the recursion carries the NaN backwards).  The last period, xs = xf, is always
// defined.  It cannot happen (in exact arithmetic) when P is positive definite: A invertible with Sigma0 positive definite
// (hodrick_prescott: det A = 1), or Q positive definite.  It does happen for a row whose second state is identically zero
// (A = diag(a, 0), Q = diag(q, 0), Sigma0 = diag(s0, 0)): P = diag(p, 0) at every step.
SMC_HD void rts2_step(const double* r, double xf1, double xf2, double F11, double F21, double F22, double& xs1, double& xs2, double& Ps11,
                      double& Ps21, double& Ps22) {
    double M[4], P11, P21, P22, p1 = xf1, p2 = xf2;
    kalman2_predict(r, p1, p2, F11, F21, F22, M, P11, P21, P22);
    const double det = fma(P11, P22, -(P21 * P21));
    const bool ok = det > 0.0 && det - det == 0.0;
    const double idet = 1.0 / det;
    const double G11 = fma(M[0], P22, -(M[2] * P21)) * idet, G12 = fma(M[2], P11, -(M[0] * P21)) * idet;
    const double G21 = fma(M[1], P22, -(M[3] * P21)) * idet, G22 = fma(M[3], P11, -(M[1] * P21)) * idet;
    const double d1 = xs1 - p1, d2 = xs2 - p2;
    const double D11 = Ps11 - P11, D21 = Ps21 - P21, D22 = Ps22 - P22;
    const double E11 = fma(G12, D21, G11 * D11), E12 = fma(G12, D22, G11 * D21);
    const double E21 = fma(G22, D21, G21 * D11), E22 = fma(G22, D22, G21 * D21);
    const double nan = bits2d(0x7ff8000000000000ULL);
    xs1 = ok ? fma(G12, d2, fma(G11, d1, xf1)) : nan;
    xs2 = ok ? fma(G22, d2, fma(G21, d1, xf2)) : nan;
    Ps11 = ok ? F11 + fma(E12, G12, E11 * G11) : nan;
    Ps21 = ok ? F21 + fma(E22, G12, E21 * G11) : nan;
    Ps22 = ok ? F22 + fma(E22, G22, E21 * G21) : nan;
}
// Simulation of such a row (simulate, state_space_models.jl:11-26).  The lower factor L of a covariance C that may be singular:
//   l11 = sqrt(C11);  l21 = C11 > 0 ? C21 / l11 : 0;  l22 = sqrt(max(C22 - l21 l21, 0))
// x_1 = x0 + L(Sigma0) z, x_t = A x_{t-1} + L(Q) z, y_t = B x_t + sqrt(R) e with z = (z0 of slot SLOT_NORMAL0, z0 of slot
// SLOT_NORMAL0 + 1) and e = z0 of slot SLOT_OBS of draw(seed, 0, SIM_STREAM, t, slot): the slots smc_simulate uses.
SMC_HD void lg2_factor(double C11, double C21, double C22, double& l11, double& l21, double& l22) {
    l11 = sqrt(C11);
    l21 = C11 > 0.0 ? C21 / l11 : 0.0;
    const double v = fma(-l21, l21, C22);
    l22 = sqrt(v > 0.0 ? v : 0.0);
}
SMC_HD void lg2_sim_step(const double* r, bool first, double z0, double z1, double e, double& x1, double& x2, double& y) {
    double l11, l21, l22, m1, m2;
    if (first) {
        lg2_factor(r[LG2_S11], r[LG2_S21], r[LG2_S22], l11, l21, l22);
        m1 = r[LG2_X1]; m2 = r[LG2_X2];
    } else {
        lg2_factor(r[LG2_Q11], r[LG2_Q21], r[LG2_Q22], l11, l21, l22);
        m1 = fma(r[LG2_A12], x2, r[LG2_A11] * x1); m2 = fma(r[LG2_A22], x2, r[LG2_A21] * x1);
    }
    x1 = fma(l11, z0, m1);
    x2 = fma(l22, z1, fma(l21, z0, m2));
    y = fma(sqrt(r[LG2_R]), e, fma(r[LG2_B2], x2, r[LG2_B1] * x1));
}

// ---- summaries of an IBIS cloud (src/plotting_utils.jl:94-137: observation_dist, estimated_trend, quantile) -----------------
// Particle m: row (A, B, Q, R), filtered state (x, S), outer log-weight logw.  With omega_m the normalised weight of logw:
//   ahead = 0:  ym = B x,        vm = (B B) S + R                         (:104-105)
//   ahead = 1:  ym = B (A x),    vm = (B B) ((A A) S + Q) + R             one prediction of kalman_step first (kalman_filter.jl:39-40)
//   y = sum omega ym, Sigma = sum omega vm (:107-108), by = sum omega (ym - y)^2   (Sigma + by: the variance of the mixture)
//   xbar = sum omega x, Sbar = sum omega S, bx = sum omega (x - xbar)^2            (the filtered state, whatever `ahead`)
// Order of operations - a function of the arrays alone.  The cloud is cut into CHUNKS of IBIS_SUM_CHUNK = 64 consecutive
// particles (the last one padded with dead lanes).  Per chunk, with exp(logw) = p 2^k (sp_exp_parts; a lane takes part iff lw_alive):
//   kc = max k;  u = p 2^(k - kc), 0 when k - kc <= -64 or the lane is dead;  a lane with u = 0 contributes +0.0 to every sum,
//                whatever its x (NaN included)
//   l* = the lowest lane with the largest u;  cy = ym[l*], cx = x[l*]        (the shifts of the chunk; 0 for a dead chunk)
//   W = sum u, Dy = sum u (ym - cy), V = sum u vm, My = sum u ((ym - cy)(ym - cy)), Dx, Sx, Mx likewise in (x, S):
//   each the TREE sum over the 64 lanes: a[i] += a[i ^ 1], then ^ 2, 4, 8, 16, 32 (a wave's butterfly; every lane ends equal)
// The chunk record is (kc, W, cy, Dy, V, My, cx, Dx, Sx, Mx), IBIS_SUM_NF doubles.  Combine, chunks LEFT TO RIGHT from 0.0:
//   K = max kc;  f_c = 2^-(K - kc), 0 when K - kc >= 64 or W_c = 0;  D = sum_c f_c W_c;  Om_c = (f_c W_c) / D
//   y     = sum_c (Om_c cy_c + (f_c Dy_c) / D)         Sigma = sum_c (f_c V_c) / D          (xbar, Sbar likewise)
//   by    = sum_c ((f_c My_c) / D + (2 e_c) ((f_c Dy_c) / D) + Om_c (e_c e_c)),  e_c = cy_c - y      (bx likewise)
// - a single pass over the cloud with one shift per chunk: every term of by is a sum of squares about a member of its own chunk
// plus the exact correction to y, so nothing cancels, and a cloud whose weight sits on one particle gives by = bx = 0 exactly.
// A chunk with f_c W_c = 0 adds nothing.  A cloud without a live particle (D = 0) gives NaN everywhere.
// out [IBIS_SUM_NOUT] = (y, Sigma, by, xbar, Sbar, bx, K, D):  logsumexp(logw) = K ln 2 + log D.
constexpr int IBIS_SUM_CHUNK = 64;
constexpr int IBIS_SUM_NF = 10;
constexpr int IBIS_SUM_NOUT = 8;
enum { ISF_KC = 0, ISF_W, ISF_CY, ISF_DY, ISF_V, ISF_MY, ISF_CX, ISF_DX, ISF_SX, ISF_MX };

constexpr int IBIS_SUM_DEADK = -(1 << 30);
// (ym, vm) of a particle
SMC_HD void ibis_obs_moments(double A, double B, double Q, double R, double x, double S, bool ahead, double& ym, double& vm) {
    if (ahead) { x = A * x; S = (A * A) * S + Q; }
    ym = B * x;
    vm = (B * B) * S + R;
}
// exp(logw) = p 2^k of a lane: k = IBIS_SUM_DEADK for a lane that takes no part
SMC_HD double ibis_sum_parts(double logw, bool valid, int& k) {
    const bool alive = valid && lw_alive(logw);
    double kd = 0.0;
    const double p = sp_exp_parts(alive ? logw : 0.0, kd);
    k = alive ? (int)kd : IBIS_SUM_DEADK;
    return alive ? p : 0.0;
}
SMC_HD double ibis_sum_u(double p, int k, int kc) { return (k != IBIS_SUM_DEADK && k - kc > -64) ? scale2(p, k - kc) : 0.0; }
// the seven addends of a lane, t = (u, u dy, u vm, u dy dy, u dx, u S, u dx dx)
SMC_HD void ibis_sum_terms(double u, double ym, double vm, double x, double S, double cy, double cx, double* t) {
    const bool on = u > 0.0;
    const double dy = ym - cy, dx = x - cx;
    t[0] = u;
    t[1] = on ? u * dy : 0.0;
    t[2] = on ? u * vm : 0.0;
    t[3] = on ? u * (dy * dy) : 0.0;
    t[4] = on ? u * dx : 0.0;
    t[5] = on ? u * S : 0.0;
    t[6] = on ? u * (dx * dx) : 0.0;
}
// g_c = f_c W_c of a chunk against the cloud's K (both integral doubles or -inf)
SMC_HD double ibis_sum_factor(double K, double kc, double W) {
    const double dk = K - kc;
    return (W > 0.0 && dk >= 0.0 && dk < 64.0) ? pow2i(-(int)dk) : 0.0;
}
// the first-moment addends of a chunk once D is known: (Om cy + f Dy / D, f V / D, Om cx + f Dx / D, f Sx / D)
SMC_HD void ibis_sum_first(const double* r /*[IBIS_SUM_NF]*/, double f, double D, double* a /*[4]*/) {
    const bool on = f * r[ISF_W] > 0.0;
    const double Om = (f * r[ISF_W]) / D;
    a[0] = on ? Om * r[ISF_CY] + (f * r[ISF_DY]) / D : 0.0;
    a[1] = on ? (f * r[ISF_V]) / D : 0.0;
    a[2] = on ? Om * r[ISF_CX] + (f * r[ISF_DX]) / D : 0.0;
    a[3] = on ? (f * r[ISF_SX]) / D : 0.0;
}
// the second-moment addends of a chunk once y and xbar are known
SMC_HD void ibis_sum_second(const double* r, double f, double D, double y, double xbar, double* b /*[2]*/) {
    const bool on = f * r[ISF_W] > 0.0;
    const double Om = (f * r[ISF_W]) / D;
    const double ey = r[ISF_CY] - y, ex = r[ISF_CX] - xbar;
    b[0] = on ? ((f * r[ISF_MY]) / D + (2.0 * ey) * ((f * r[ISF_DY]) / D)) + Om * (ey * ey) : 0.0;
    b[1] = on ? ((f * r[ISF_MX]) / D + (2.0 * ex) * ((f * r[ISF_DX]) / D)) + Om * (ex * ex) : 0.0;
}

// ---- the RTS smoother of an IBIS cloud (Rauch, Tung and Striebel 1965) -----------------------------------------
// Particle m has the row (A, B, Q, R, x0, sigma0).  Its filtered record (xf_t, Sf_t), t = 0..T-1, is what kalman_step leaves
// after step t from (x0, sigma0): step 0 predicts iff predict_first, every later step predicts.  The backward pass, t = T-2 .. 0
// from xs_{T-1} = xf_{T-1}, Ps_{T-1} = Sf_{T-1}, in this order of operations (rts_gain, rts_back):
//   Sp = (A A) Sf_t + Q                          the predicted variance of step t+1, as kalman_step forms it
//   G  = Sp > 0 ? (Sf_t A) / Sp : 0
//   V  = Sp > 0 ? (Sf_t Q) / Sp : Sf_t           the variance of x_t given x_{t+1} and y_1:t
//   xs_t = xf_t + G (xs_{t+1} - A xf_t)
//   Ps_t = V + (G G) Ps_{t+1}                    a sum of non-negative terms (Sf + G^2 (Ps' - Sp) would cancel)
// The cloud at period t is integrated by "summaries of an IBIS cloud" above with ahead = 0, (x, S) := (xs_t, Ps_t) and the
// particle's own logw: the same chunks, tree and left-to-right combine, so row t of the output is the eight numbers of
// smc_ibis_summary, now the smoothed fitted observation and the smoothed state.
// Paths: path p (0-based) belongs to parameter particle m = which[p] and is, from t = T-1 down,
//   x_{T-1} = xf_{T-1} + sd(Sf_{T-1}) z
//   x_t     = (xf_t + G (x_{t+1} - A xf_t)) + sd(V) z,    sd(v) = v > 0 ? sqrt(v) : 0  (correctly rounded)
//   z       = box_muller(draw(path_seed, p >> 1, stream = which[p], t, SLOT_RTS)): z0 for an even p, z1 for an odd one
// so a path is a function of (row, y, path_seed, p, which[p]) alone: not of the number of paths, the cloud or the launch.
constexpr uint32_t SLOT_RTS = 36u;                // no other draw uses it (SLOT_PATH is 35; the others end at 34)
SMC_HD void rts_gain(double A, double Q, double Sf, double& G, double& V) {
    const double Sp = (A * A) * Sf + Q;
    const bool on = Sp > 0.0;
    G = on ? (Sf * A) / Sp : 0.0;
    V = on ? (Sf * Q) / Sp : Sf;
}
// (xs, Ps) of step t+1 in, of step t out
SMC_HD void rts_back(double A, double Q, double xf, double Sf, double& xs, double& Ps) {
    double G, V;
    rts_gain(A, Q, Sf, G, V);
    xs = xf + G * (xs - A * xf);
    Ps = V + (G * G) * Ps;
}
SMC_HD double rts_sd(double v) { return v > 0.0 ? sqrt(v) : 0.0; }
SMC_HD double rts_normal(uint64_t seed, int64_t p, uint32_t stream, uint32_t t) {
    double z0, z1;
    box_muller(draw(seed, (uint32_t)(p >> 1), stream, t, SLOT_RTS), z0, z1);
    return (p & 1) ? z1 : z0;
}
SMC_HD double rts_path_last(double xf, double Sf, double z) { return xf + rts_sd(Sf) * z; }
// x_{t+1} of the path in, x_t out
SMC_HD double rts_path_back(double A, double Q, double xf, double Sf, double xnext, double z) {
    double G, V;
    rts_gain(A, Q, Sf, G, V);
    return (xf + G * (xnext - A * xf)) + rts_sd(V) * z;
}

// ---- moments of the theta cloud of an IBIS sampler (random_walk_kernel, smc_samplers.jl:87-101; expected_parameters, ibis.jl:60-64) --
// theta [M][d], outer log-weights logw [M].  Two modes, one order of operations - a function of the arrays alone:
//   unweighted:  c_m = 1 for every particle;                       mean = (sum theta) / M,   cov = (sum dd') / (M - 1)  (corrected)
//   weighted:    c_m = u_m / W, u_m = p_m 2^(k_m - K), W = sum u;  mean = sum c theta,       cov = sum c dd'            (uncorrected)
// with d = theta - mean (the CENTRED second pass), exp(logw) = p 2^k (ibis_sum_parts; a particle takes part iff lw_alive),
// K = max k over the live particles (an integer maximum: any order) and u = 0 for a dead particle or k - K <= THETA_MOM_MINK.
// A particle with u = 0 contributes +0.0 to every sum whatever its theta (NaN included).  Every sum - W, then the d sums of
// c theta_i, then the d (d + 1) / 2 sums of c (d_i d_j), j <= i - is taken the way the summaries above take theirs: CHUNKS of
// IBIS_SUM_CHUNK = 64 consecutive particles (the last one padded with +0.0), the butterfly TREE a[i] += a[i ^ 1], ^ 2, .., ^ 32
// within a chunk, the chunks LEFT TO RIGHT from 0.0.  The weights are normalised before they multiply (c = u / W), so a cloud
// whose weight sits on one particle has c = 1 there: mean = that theta exactly and cov = 0 exactly.  W = 0 (no live particle), and
// M = 1 in the unweighted mode, give NaN.  smc_host_theta_moments is this paragraph on the host, smc_ibis_theta_moments on the device.
constexpr int THETA_MOM_MINK = -960;     // (u / W stays a normal number: W < 2^31)
constexpr int THETA_MOM_NTRI = MAX_DTHETA * (MAX_DTHETA + 1) / 2;
SMC_HD double theta_mom_u(double p, int k, int K) { return (k != IBIS_SUM_DEADK && k - K > THETA_MOM_MINK) ? scale2(p, k - K) : 0.0; }
// the addend of a particle with coefficient c (on: it takes part) for the value v
SMC_HD double theta_mom_term(bool on, double c, double v) { return on ? c * v : 0.0; }
// what a finished sum s becomes: s / div when div_on (NaN for div = 0), and NaN for a weighted cloud without a live particle
SMC_HD double theta_mom_finish(double s, bool div_on, double div, bool weighted, double W) {
    const double nan = bits2d(0x7ff8000000000000ULL);
    if (div_on) s = div > 0.0 ? s / div : nan;
    if (weighted) s = W > 0.0 ? s : nan;
    return s;
}

// ---- quantiles and histograms of the theta cloud (construct_histograms, src/plotting_utils.jl:5-37) -----------------------------
// theta [M][d], outer log-weights logw [M].  Everything is INTEGER arithmetic on values derived per particle, so the result is a
// function of the arrays alone - any launch geometry, any order of evaluation, host and device the same bits.
//   weight   (p_m, k_m) = ibis_sum_parts(logw_m), K = max k_m over the live particles (the K of the moments above),
//            q_m = fix_weight_i(p_m, k_m - K, THETA_Q_BITS); a dead particle (!lw_alive) has q_m = 0 whatever its theta.
//            sp_exp_parts returns p in [0.707, 1.415], so q_m <= 1.415 2^32 < 2^32.51 and W = sum q_m < 2^62.51 at M = 2^30: W
//            fits 63 bits (and p 2^32 < 2^50 is what fix_weight_i asks for).  A live particle with k_m = K has q_m >= 0.707 2^32,
//            so W > 0 exactly when some particle is alive, and then W >= 2^(THETA_Q_BITS - 1).
//   order    the IEEE total order of the bits (smc_host_quantile7): order_key (smc_kernels.h) maps a double to a uint64 that
//            compares the same way, key_value maps it back: -NaN < -inf < .. < -0.0 < +0.0 < .. < +inf < +NaN.  A NaN theta
//            that carries weight sorts by its sign bit.
//   quantile of coordinate i at level p: the smallest v among theta[.][i] with sum{q_m : key(theta_mi) <= key(v)} > T,
//            T = umulhi64(prob_to_u64(p), W) < W (smc_get_quantiles' definition): p = 0 the smallest value that carries weight,
//            p = 1 the largest, no interpolation.  W = 0: NaN at every level.
//   histogram of coordinate i over [lo, hi) in nbins equal bins, scale = nbins / (hi - lo) computed once in double: slot 0
//            "under" (theta < lo), slots 1 .. nbins the bins (min((int)((theta - lo) scale), nbins - 1): the ms_bin rule), slot
//            nbins + 1 "over" (theta >= hi), slot nbins + 2 "nan".  counts [nbins + 3] are the sums of q_m: they add up to W.
constexpr int THETA_Q_BITS = 32;
constexpr int THETA_HIST_MAXBINS = 4096;
SMC_HD uint64_t theta_q(double p, int k, int K) { return k != IBIS_SUM_DEADK ? fix_weight_i(p, k - K, THETA_Q_BITS) : 0; }
// the range of a histogram: lo < hi, both finite, and a finite width (so that scale > 0 and (theta - lo) scale is a number)
SMC_HD bool theta_hist_range_ok(double lo, double hi) {
    const double w = hi - lo;
    return lo < hi && w < inf() && lo > -inf() && hi < inf();
}
SMC_HD int theta_hist_slot(double v, double lo, double hi, double scale, int nbins) {
    if (v != v) return nbins + 2;
    if (v < lo) return 0;
    if (v >= hi) return nbins + 1;
    const int b = (int)((v - lo) * scale);
    return 1 + (b < nbins - 1 ? b : nbins - 1);
}

// ---- segment combine (integers only) ----------------------------------------------------------
// A segment record is (kb, S, S2): kb = max k_i of the segment (integral double, -inf if the segment
// has no live particle), S = sum q, S2 = sum q^2 (128 bit).  With K = max kb:
//   sh_b = (K - kb) + SH            right shift that brings segment b to the common scale 2^K
//   Q_b  = S_b  >> sh_b             entry of the segment table (uint64, total < 2^63)
//   R_b  = S2_b >> (2 (K-kb) + 49 + SH)
SMC_HD int table_shift_extra(int64_t npad) {
    const int s = ceil_log2_i64(npad) - 14;
    return s > 0 ? s : 0;
}
SMC_HD int seg_shift(double K, double kb, int SH) {
    const double dk = K - kb;   // >= 0 integral; inf or nan for a dead segment / dead filter
    int sh = (dk >= 0.0 && dk < 64.0) ? (int)dk + SH : 64;
    return sh > 64 ? 64 : sh;
}
SMC_HD uint64_t shr128(uint64_t hi, uint64_t lo, int s) {   // low 64 bits of (hi:lo) >> s, 0 < s < 128
    return s >= 64 ? (hi >> (s - 64)) : ((lo >> s) | (hi << (64 - s)));
}
SMC_HD uint64_t seg_Q(uint64_t S, int sh) { return sh < 64 ? S >> sh : 0; }
SMC_HD uint64_t seg_R(uint64_t S2hi, uint64_t S2lo, int sh, int SH) {
    const int sh2 = 2 * (sh - SH) + 49 + SH;
    return (sh < 64 && sh2 < 128) ? shr128(S2hi, S2lo, sh2) : 0;
}
SMC_HD void combine_outputs(double K, uint64_t Dtot, uint64_t Rtot, int SH, int64_t n, double& logmu, double& ess) {
    const double Dd = (double)Dtot * pow2i(SH - 48), Rd = (double)Rtot * pow2i(SH - 47);
    logmu = Dtot ? fma(K, LN2_HI, fma(K, LN2_LO, sp_log(Dd))) - sp_log((double)n) : -inf();
    ess = Rtot ? Dd * Dd / Rd : 0.0;
}

// ---- the smoother: forward filtering, backward smoothing ------------------------------------------------------
// Given the clouds (x_t, w_t), t = 1..T, of a step-by-step run (w the dense weights of smc_get_state) the smoothed weights are
//     ws_T = w_T,   and for t = T-1 .. 1, with "source" l, i a particle of step t and "target" j a particle of step t+1:
//     a_lj   = fma chain of logf(x_{t+1}^j | x_t^l) started from g_l = sp_log(w_t^l) + c_l        (log w + logf, one constant)
//     M_j    = max_l a_lj,   S_j = sum_l sp_exp(a_lj - M_j),   logD_j = M_j + sp_log(S_j)
//     ws_t^i = w_t^i > 0 ? w_t^i * sum_j ws_{t+1}^j * sp_exp(logf(x_{t+1}^j | x_t^i) - logD_j) : 0
// Sources with w = 0 and targets with ws = 0 (NaN compares false: they count as 0) are left out of every sum and maximum,
// whatever their states; there is no renormalisation.  Order: the summed index is cut into chunks of SMOOTH_CH consecutive
// particles; a chunk is summed in ascending index order with plain adds starting from +0.0, the chunk partials are summed in
// ascending order starting from +0.0; the maximum is exact in any order.  (The kernels give a left-out particle the log-weight
// -inf resp. the weight 0 and logD = +inf with a zero state: its terms are exactly +0.0, which changes no partial sum.)
// logf is split into what depends on the source alone (centres m, the scale s, the constant c) and a chain of fma over the pair:
//   LG1D    m = A xp,  s = nh0 = -0.5 / Q,  c = c0 = -HALF_LOG2PI - sp_log(sqrt(Q))
//   SV1D    m = fma(rho, xp - mu, mu),  s = nh0 = -0.5 / (sigma sigma),  c = c0 = -HALF_LOG2PI - sp_log(sigma)
//   UCSV3D  m = xp (three rows),  s = -0.5 sp_exp(-xp[1]),  c = fma(-0.5, xp[1], c0),  nh1 = -0.5 / (g_eps g_eps),
//           nh2 = -0.5 / (g_eta g_eta),  c0 = ((-HALF_LOG2PI - sp_log(g_eps)) + (-HALF_LOG2PI - sp_log(g_eta))) - HALF_LOG2PI
//           (the reference's conventions: the trend moves with the PREVIOUS lse, sd exp(lse / 2); the gammas are standard deviations)
//   pair    d_r = x[r] - m[r];   one row: fma(d0 d0, s, g);   UCSV3D: fma(d0 d0, s, fma(d1 d1, nh1, fma(d2 d2, nh2, g)))
// with g = c for logf itself and g = sp_log(w) + c for a_lj.  MODEL_UCSV_RB has no transition density of its rows (m and P are
// functions of the whole path): no smoother of this kind; "Rao-Blackwellised backward simulation" below is its smoother.
#ifndef SMC_SMOOTH_CH
#define SMC_SMOOTH_CH 128
#endif
constexpr int SMOOTH_CH = SMC_SMOOTH_CH;   // 64, 128 or 256 (profiles/smoother_cost.log); part of the numerical contract
static_assert(SMOOTH_CH == 64 || SMOOTH_CH == 128 || SMOOTH_CH == 256, "SMOOTH_CH: 64, 128 or 256");
struct SmoothRow {   // the constants of a parameter row, derived once per filter on the host
    double a, mu, nh0, nh1, nh2, c0;
};
// false: the family has no transition density, or the row's transition scale is not a positive finite number (host only)
inline bool smooth_row(int model, const double* raw, SmoothRow& k) {
    k = SmoothRow{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    auto scale_ok = [](double s) { return s == s && s > 0.0 && s != inf(); };
    if (model == MODEL_LG1D) {
        if (!scale_ok(raw[2])) return false;
        k.a = raw[0];
        k.nh0 = -0.5 / raw[2];
        k.c0 = -HALF_LOG2PI - sp_log(sqrt(raw[2]));
        return true;
    }
    if (model == MODEL_SV1D) {
        if (!scale_ok(raw[2])) return false;
        k.a = raw[1]; k.mu = raw[0];
        k.nh0 = -0.5 / (raw[2] * raw[2]);
        k.c0 = -HALF_LOG2PI - sp_log(raw[2]);
        return true;
    }
    if (model == MODEL_UCSV3D) {
        if (!scale_ok(raw[0]) || !scale_ok(raw[1])) return false;
        k.nh1 = -0.5 / (raw[0] * raw[0]);
        k.nh2 = -0.5 / (raw[1] * raw[1]);
        k.c0 = ((-HALF_LOG2PI - sp_log(raw[0])) + (-HALF_LOG2PI - sp_log(raw[1]))) - HALF_LOG2PI;
        return true;
    }
    return false;
}
// what logf(. | xp) needs of the source xp alone
template <int MODEL>
SMC_HD void logf_source(const SmoothRow& k, const double* xp, double* m /*[d]*/, double& s, double& c) {
    if constexpr (MODEL == MODEL_LG1D) {
        m[0] = k.a * xp[0]; s = k.nh0; c = k.c0;
    } else if constexpr (MODEL == MODEL_SV1D) {
        m[0] = fma(k.a, xp[0] - k.mu, k.mu); s = k.nh0; c = k.c0;
    } else {
        m[0] = xp[0]; m[1] = xp[1]; m[2] = xp[2];
        s = -0.5 * sp_exp(-xp[1]);
        c = fma(-0.5, xp[1], k.c0);
    }
}
// g + (logf(x | xp) - c): the chain over the pair
template <int MODEL>
SMC_HD double logf_pair(const SmoothRow& k, const double* m, double s, double g, const double* x) {
    const double d0 = x[0] - m[0];
    if constexpr (MODEL == MODEL_UCSV3D) {
        const double d1 = x[1] - m[1], d2 = x[2] - m[2];
        return fma(d0 * d0, s, fma(d1 * d1, k.nh1, fma(d2 * d2, k.nh2, g)));
    } else {
        return fma(d0 * d0, s, g);
    }
}
// logpdf(transition(model, xp), x)          ssm.jl:87-94, 233-242
template <int MODEL>
SMC_HD double model_logf(const SmoothRow& k, const double* xp, const double* x) {
    double m[3], s, c;
    logf_source<MODEL>(k, xp, m, s, c);
    return logf_pair<MODEL>(k, m, s, c, x);
}
// sum of n terms term(i), i = 0..n-1, in the smoother's order (chunks of SMOOTH_CH, plain adds, partials in ascending order)
template <class F>
inline double smooth_sum(int64_t n, F term) {
    double tot = 0.0;
    for (int64_t c0 = 0; c0 < n; c0 += SMOOTH_CH) {
        double s = 0.0;
        const int64_t c1 = c0 + SMOOTH_CH < n ? c0 + SMOOTH_CH : n;
        for (int64_t i = c0; i < c1; ++i) s += term(i);
        tot += s;
    }
    return tot;
}

// ---- the smoother: lag-one pair moments ----------------------------------------------------------------------------
// The quantities of the smoother above: source i at step t, target j at step t+1, d state rows, and the centres m_c(x_t^i) of
// logf_source (LG1D: A x;  SV1D: fma(rho, x - mu, mu);  UCSV3D: x in all three rows).  For t = 0 .. T-2:
//     p_ij  = ws_{t+1}^j * sp_exp(logf(x_{t+1}^j | x_t^i) - logD_j)                  (pair_prob: bit for bit the term ws_t^i sums)
//     X_i^c = sum_j p_ij * x_{t+1}^{j,c}                                              (pair_x_term)
//     R_i^c = sum_j p_ij * (d_c * d_c),   d_c = x_{t+1}^{j,c} - m_c(x_t^i)           (pair_r_term: the d_r of logf_pair, same bits)
//     cross[t][a][c] = sum_i (w_t^i * x_t^{i,a}) * X_i^c      -> E[x_t^a x_{t+1}^c | y_1:T]                     (pair_cross_term)
//     resid2[t][c]   = sum_i  w_t^i * R_i^c                   -> E[(x_{t+1}^c - m_c(x_t))^2 | y_1:T]            (pair_resid_term)
// The sums over j run in the smoother's order (chunks of SMOOTH_CH, plain adds from +0.0, partials in ascending order), the sums
// over i in smooth_sum's.  A target with ws = 0 and a source with w = 0 (NaN compares false) contribute exactly +0.0 whatever
// their states: by a select, not by a product with zero, on the owner side as well.  (The kernels stage a left-out target as the
// smoother does - weight 0, logD = +inf, a zero state - so that its three terms are exactly +0.0, and select on w in the kernel
// that finishes a step.)  There is no renormalisation; a filter that collapsed at any recorded step reads NaN everywhere; T = 1
// has no pair.  MODEL_UCSV_RB has no pair moments, as it has no smoother of this kind.
template <int MODEL>
SMC_HD double pair_prob(const SmoothRow& k, const double* m, double s, double c, const double* xj, double wsj, double logDj) {
    return wsj * sp_exp(logf_pair<MODEL>(k, m, s, c, xj) - logDj);
}
SMC_HD double pair_x_term(double p, double xjc) { return p * xjc; }
SMC_HD double pair_r_term(double p, double xjc, double mc) {
    const double dc = xjc - mc;
    return p * (dc * dc);
}
SMC_HD double pair_cross_term(double wi, double xia, double Xc) { return wi > 0.0 ? (wi * xia) * Xc : 0.0; }
SMC_HD double pair_resid_term(double wi, double Rc) { return wi > 0.0 ? wi * Rc : 0.0; }

// ---- the smoother: quantiles of the smoothed state -----------------------------------------------------------------
// The quantile of ONE cloud: n values x_i (one state coordinate of one recorded step of one filter) with the smoothed weights
// ws_i, non-negative doubles that nothing has normalised.  After the per-particle conversion below everything is INTEGER
// arithmetic, so the result is a function of the two arrays alone: any launch geometry, any order of evaluation, host and
// device the same bits.
//   who takes part   particle i iff 0 < ws_i < +inf (smooth_q_takes_part; NaN compares false).  Its state may be anything, NaN
//            included; the state of a particle that does not take part is never looked at.
//   no quantile      no particle takes part, or some ws_i is NaN (a filter that collapsed at a recorded step: smc_smooth writes
//            NaN everywhere): every level is NaN.
//   weight   ws_i = f_i 2^(e_i), f_i in [0.5, 1) (smooth_q_parts: the bits of the double, a subnormal normalised by its leading
//            zeros, so exact for every positive finite double); K = max e_i over the particles that take part;
//            q_i = fix_weight_i(f_i, e_i - K, SMOOTH_Q_BITS) = rint(ws_i 2^(SMOOTH_Q_BITS - K)), ties to even (below e_i - K =
//            -(SMOOTH_Q_BITS + 2) the 0 that fix_weight_i returns is what the rounding gives).  A particle that does not take
//            part has q_i = 0.
//   SMOOTH_Q_BITS = 40: the largest value for which W = sum q_i fits 63 bits at the largest cloud the smoother admits, 65535
//            chunks of 128 = 8388480 < 2^23 particles, each q_i <= 2^40 (f < 1): W <= 8388480 2^40 < 2^63.  (f 2^40 < 2^50 is
//            what fix_weight_i asks for.)  The particle with e_i = K has q_i >= 2^39, so W >= 2^39 > 0 whenever somebody takes
//            part.  Each q_i is within half a unit of ws_i 2^(40 - K) and sum ws_i 2^(-K) >= 1/2, so every cumulative share
//            of W differs from the share of the dense weights by at most n 2^(2 - SMOOTH_Q_BITS) (tests/test_smooth_quantiles_host.py
//            derives and checks it): 2^-28 at 1024 particles.
//   order    the IEEE total order of the bits: order_key / key_value (smc_kernels.h), as smc_host_quantile7 and the theta
//            quantiles use it: -NaN < -inf < .. < -0.0 < +0.0 < .. < +inf < +NaN.  A NaN state that carries weight sorts by its
//            sign bit.
//   level p in [0, 1]: T = mulhi64(prob_to_u64(p), W) < W; the quantile is the smallest v among the x_i with
//            sum{q_i : key(x_i) <= key(v)} > T (smc_get_quantiles' definition): p = 0 the smallest value that carries weight,
//            p = 1 the largest, no interpolation.
constexpr int SMOOTH_Q_BITS = 40;
constexpr int SMOOTH_Q_NOBODY = -(1 << 30);   // K of a cloud in which nobody takes part
SMC_HD bool smooth_q_takes_part(double ws) { return ws > 0.0 && ws < inf(); }
// (f, e) of a positive finite ws = f 2^e, f in [0.5, 1): exact, subnormals included
SMC_HD double smooth_q_parts(double ws, int& e) {
    uint64_t b = d2bits(ws);
    int E = (int)(b >> 52);                                // (the sign bit is 0)
    if (E == 0) {                                          // a subnormal m 2^-1074, 0 < m < 2^52: its leading bit to bit 52
        const int sh = __builtin_clzll(b) - 11;
        b <<= sh;
        E = 1 - sh;
    }
    e = E - 1022;
    return bits2d((b & 0x000fffffffffffffULL) | 0x3fe0000000000000ULL);
}
// e_i of a particle, SMOOTH_Q_NOBODY when it does not take part: K is the maximum of these
SMC_HD int smooth_q_exponent(double ws) {
    int e = SMOOTH_Q_NOBODY;
    if (smooth_q_takes_part(ws)) (void)smooth_q_parts(ws, e);
    return e;
}
SMC_HD uint64_t smooth_q_weight(double ws, int K) {
    if (!smooth_q_takes_part(ws)) return 0;
    int e;
    const double f = smooth_q_parts(ws, e);
    return fix_weight_i(f, e - K, SMOOTH_Q_BITS);
}

// ---- backward simulation: joint smoothing paths (FFBSi; Godsill, Doucet and West 2004) --------------------------
// Inputs: the recorded clouds (x_t, w_t), t = 0..T-1, of one filter (w the dense weights), its SmoothRow, a path seed and the
// filter's Philox stream id.  Path p (0-based) is a function of these alone: not of the number of paths, of the other paths,
// of the batch or of any launch geometry.  For t = T-1 .. 0, with j = idx[t+1][p] when t < T-1:
//   a source l is live iff w_t^l > 0 (NaN compares false)
//   b_l = sp_log(w_t^l)                                    at the last step
//   b_l = logf_pair(k, m_l, s_l, g_l, x_{t+1}^j),  (m_l, s_l, c_l) = logf_source(x_t^l),  g_l = sp_log(w_t^l) + c_l   before it
//         (bit for bit the a_lj of the smoother)
//   M_p = max of b_l over the live sources, taken with b > M ? b : M from -inf (a NaN is dropped; exact in any order)
//   q_l = path_weight(b_l, M_p): with e = b_l - M_p and (pp, kk) = sp_exp_parts(e), fix_weight(pp, kk, PATH_BITS) when e <= 0,
//         else 0 (a NaN b_l, an infinite M_p); 0 for a source that is not live.  The heaviest source has e = 0: q = 2^PATH_BITS
//   S   = sum of q_l, an INTEGER sum (exact in any order and any split); n <= PATH_MAX_N keeps it below 2^61
//   u   = a 64-bit half of draw(path_seed, p >> 1, stream, t, SLOT_PATH): v[1] << 32 | v[0] for an even p, v[3] << 32 | v[2] for
//         an odd one (the convention of the outer level's pick numbers)
//   r   = the high 64 bits of the 128-bit product u S
//   idx[t][p] = the smallest i with C_i > r, C_i = sum_{l <= i} q_l in ascending index order; the path's state is x_t^i, copied
// A path ends where S = 0 (no live source reaches the target: M_p = -inf): index -1 and NaN states there and at every earlier
// step.  A filter that collapsed at any recorded step (every weight 0 there; the smoother's dead flag) has -1 / NaN everywhere.
// The marginal law of idx[t][p] given the clouds is the smoothed weight ws_t of the smoother, up to the 2^-PATH_BITS grid.
constexpr int PATH_BITS = 40;
constexpr uint32_t SLOT_PATH = 35u;               // no other draw uses it (the step, PMMH and outer-level slots end at 34)
constexpr int64_t PATH_MAX_N = (int64_t)1 << 20;  // particles per filter: S < 2^61
SMC_HD uint64_t path_weight(double b, double M) {
    const double e = b - M;
    double kk;
    const double pp = sp_exp_parts(e, kk);
#if defined(__HIP_DEVICE_COMPILE__)
    // branch-free: the exponent is clamped to fix_weight's range BEFORE the conversion (a NaN becomes the lower end), the value
    // is rounded and converted by one addition as in fix_weight_i, and the two conditions select afterwards
    double kc = kk >= -(double)(PATH_BITS + 2) ? kk : -(double)(PATH_BITS + 2);
    kc = kc <= 0.0 ? kc : 0.0;
    const uint64_t q = d2bits(scale2(pp, PATH_BITS + (int)kc) + 0x1p52) & 0x000fffffffffffffULL;
    return (e <= 0.0 && kk >= -(double)(PATH_BITS + 2)) ? q : 0;
#else
    if (!(e <= 0.0)) return 0;
    return fix_weight(pp, kk, PATH_BITS);
#endif
}
// the 64-bit uniform of path p at step t
SMC_HD uint64_t path_uniform(uint64_t seed, int64_t p, uint32_t stream, uint32_t t) {
    const u32x4 v = draw(seed, (uint32_t)(p >> 1), stream, t, SLOT_PATH);
    return (p & 1) ? ((uint64_t)v.v[3] << 32) | v.v[2] : ((uint64_t)v.v[1] << 32) | v.v[0];
}
SMC_HD uint64_t mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// ---- Rao-Blackwellised backward simulation (Lindsten, Bunch, Saerkkae, Schoen and Godsill 2016) ---------------
// MODEL_UCSV_RB has no transition density of its four rows, but its two log-volatilities are an autonomous Markov chain and the
// trend is linear-Gaussian given their path.  So the walk of "backward simulation" above runs over the VOLATILITIES alone, with
// the trend integrated out on both sides: forward by the rows (m, P) the filter recorded, backward by one scalar information
// recursion per path.  Inputs: the recorded clouds (rows (m, lse, lsn, P), the posterior after y_t; dense weights w_t),
// t = 0..T-1, of one filter, UCSV's parameter row (g_eps, g_eta, x0, lse0, lsn0), y, a path seed and the filter's Philox stream
// id.  Path p is a function of these alone: not of M, the other paths, the batch or the launch geometry.
// THE WALK, t = T-1 .. 0.  The owner holds (a+, b+, mu, tau): the lse and lsn of the particle chosen at t+1, and the information
// of y_{t+1:T} about x_{t+1} as a pseudo-observation mu of x_{t+1} with variance tau.
//   a source l is live iff w_t^l > 0
//   staged (rb_source): (m_l, V_l = P_l + sp_exp(lse_l), lse_l, lsn_l, g_l = sp_log(w_t^l));  V_l is the predictive variance of
//         x_{t+1}.  At the last step (0, 0, 0, 0, g_l), and the owner reads (0, 0, 0, 1): the chain below returns g_l exactly
//   b_l = rb_pair: with d1 = a+ - lse_l, d2 = b+ - lsn_l, e = mu - m_l, D = V_l + tau, nh1 = -0.5 / g_eps^2, nh2 = -0.5 / g_eta^2,
//         fma(d1 d1, nh1, fma(d2 d2, nh2, fma(-0.5, sp_log(D), fma(-0.5, (e e) / D, g_l))))        ONE log and ONE division;
//         NaN when D is not a positive finite number: such a source is left out (q = 0, never the maximum).  The terms common
//         to all sources (-log g_eps - log g_eta - 3 HALF_LOG2PI) are dropped
//   M_p, q_l = path_weight(b_l, M_p), S, u = path_uniform(seed, p, stream, t), r and idx[t][p] exactly as in backward simulation
//   after the pick i (rb_info), R = sp_exp(lsn_i):
//         last step:  mu <- y_t,  tau <- R
//         before it:  tau' = tau + sp_exp(lse_i);  K = R / (R + tau');  mu <- fma(K, mu - y_t, y_t);  tau <- min(K tau', R)
//   vol[t][.][p] = (lse_i, lsn_i)
// Zero-weight sources are never chosen whatever their states; a path with S = 0 reads -1 / NaN from there back; a filter that
// collapsed at any recorded step reads -1 / NaN everywhere.
// THE TREND PASS, once per complete path (idx[0][p] >= 0), serial in t.  Forward (rb_trend_step, model_marginal_step's order):
//   Q = sp_exp(t == 0 ? lse0 : lse_{t-1});  (m-, P-) = t == 0 ? (x0, Q) : (m_{t-1}, P_{t-1} + Q);  R = sp_exp(lsn_t)
//   S = P- + R;  iS = 1 / S;  K = P- iS;  m_t = fma(K, y_t - m-, m-);  P_t = min(K R, P-)
// then rts_back(A = 1, Q = sp_exp(lse_t), m_t, P_t) from (m_{T-1}, P_{T-1}) gives tmean[t][p], tvar[t][p], and the joint draw
//   tdraw[T-1] = rts_path_last(m, P, z),  tdraw[t] = rts_path_back(1, sp_exp(lse_t), m_t, P_t, tdraw[t+1], z)
//   z = box_muller(draw(seed, p >> 1, stream, t, SLOT_RB_TREND)): z0 for an even p, z1 for an odd one
// (x_t = m_t + G (x_{t+1} - m_t) + sqrt(G Q) z with G = P_t / P-_{t+1}; G Q is formed as (P_t Q) / P-_{t+1}, rts_gain's V.)
// An incomplete path reads NaN at every t.
// THE SUMMARY over the complete paths p < count of one filter, per step: out[t][0..7] = mean of tmean, mean of tvar (within),
// population variance of tmean (between), mean and population variance of lse, of lsn, the number of complete paths.  Every sum
// runs in the smoother's order (smooth_sum over p: chunks of SMOOTH_CH, ascending; an incomplete path adds +0.0), is divided by
// the count, and the variances are CENTRED second passes.  No complete path: NaN, and the count 0.
constexpr uint32_t SLOT_RB_TREND = 37u;           // no other draw uses it (SLOT_PATH is 35, SLOT_RTS 36)
constexpr int RB_NV = 5;                          // doubles staged per source
SMC_HD void rb_source(bool last, const double* xs /*(m, lse, lsn, P)*/, double wl, double* v /*[RB_NV]*/) {
    v[0] = last ? 0.0 : xs[0];
    v[1] = last ? 0.0 : xs[3] + sp_exp(xs[1]);
    v[2] = last ? 0.0 : xs[1];
    v[3] = last ? 0.0 : xs[2];
    v[4] = sp_log(wl);
}
SMC_HD double rb_pair(const SmoothRow& k, const double* v /*[RB_NV]*/, const double* o /*(a+, b+, mu, tau)*/) {
    const double d1 = o[0] - v[2], d2 = o[1] - v[3], e = o[2] - v[0], D = v[1] + o[3];
    const bool ok = D > 0.0 && D < inf();
    const double Ds = ok ? D : 1.0;
    const double b = fma(d1 * d1, k.nh1, fma(d2 * d2, k.nh2, fma(-0.5, sp_log(Ds), fma(-0.5, (e * e) / Ds, v[4]))));
    return ok ? b : bits2d(0x7ff8000000000000ULL);
}
// (mu, tau): the information about x_{t+1} in, about x_t out, once the particle (lse, lsn) of step t is chosen
SMC_HD void rb_info(bool last, double lse, double lsn, double y, double& mu, double& tau) {
    const double R = sp_exp(lsn);
    const double tp = tau + sp_exp(lse), K = R / (R + tp), Kt = K * tp;
    mu = last ? y : fma(K, mu - y, y);
    tau = last ? R : (Kt < R ? Kt : R);
}
// (m, P) of step t-1 in (not read when first), of step t out
SMC_HD void rb_trend_step(const double* raw, bool first, double lse_prev, double lsn, double y, double& m, double& P) {
    const double Q = sp_exp(first ? raw[3] : lse_prev);
    const double m0 = first ? raw[2] : m, Pm = first ? Q : P + Q;
    const double R = sp_exp(lsn);
    const double S = Pm + R, iS = 1.0 / S, e = y - m0;
    const double K = Pm * iS, KR = K * R;
    m = fma(K, e, m0);
    P = KR < Pm ? KR : Pm;
}
SMC_HD double rb_trend_normal(uint64_t seed, int64_t p, uint32_t stream, uint32_t t) {
    double z0, z1;
    box_muller(draw(seed, (uint32_t)(p >> 1), stream, t, SLOT_RB_TREND), z0, z1);
    return (p & 1) ? z1 : z0;
}

// ---- the conditional particle filter (opt-in per handle: SMC_FLAG_CONDITIONAL) ---------------------------------
// Andrieu, Doucet and Holenstein (2010): the bootstrap filter with ONE particle of every step pinned to a reference trajectory
// xref [T][d].  With one backward-simulated path drawn from its record it is a Markov kernel on trajectories that leaves
// p(x_1:T | y_1:T, theta) invariant for any n >= 2 (particle Gibbs with backward simulation; Whiteley; Lindsten and Schoen).
// At every time index t, the first step included, the step is the ordinary bootstrap step - the same Philox slots: the other
// slots' ancestors, the state normals in the pair convention, the masking of a ragged last segment, the segment normalisation,
// the records, the emission, the time index - with one slot overridden:
//   k*_t = cond_slot(seed, stream, t, n) = mulhi64(u, n),  u = v[1] << 32 | v[0] of draw(seed, 0, stream, t, SLOT_COND)
//          one draw per filter and step, workgroup-uniform; k*_t < n, never a masked child
//   x_t^{k*}    = xref[t], copied bit for bit (the transition of that slot is computed and discarded, its normal with it)
//   logw_t^{k*} = model_logobs(prm, xref[t], y_t)
//   ancestor    = k*_{t-1}, recomputed from the draw of step t - 1 (k*_0 at t = 0); recorded with SMC_FLAG_ANCESTORS only
// WHY THE SLOT IS RANDOM.  The multinomial resampler is block-sorted: child j takes the j-th order statistic of n uniforms.
// Overriding a FIXED slot (say the last) leaves the n - 1 smallest of n draws, which are not n - 1 iid draws; dropping a
// uniformly random slot leaves n - 1 iid draws as a multiset, and only the multiset matters, because backward simulation
// ignores labels.  Bootstrap families with a transition density only (LG1D, SV1D, UCSV3D), multinomial resampling, no gaps.
// The draw is workgroup-uniform, so the kernels want it on the scalar unit: philox4x32_10's words by plain integer operators
// (its xor3 is v_bitop3_b32, a vector instruction, and drags the ten rounds - 64 quarter-rate multiplies per wave - into the
// vector unit with it).  The same integers; tests/test_conditional_host.py pins cond_slot to smc_host_philox4x32_10.
SMC_HD uint32_t cond_slot(uint64_t seed, uint32_t stream, uint32_t t, uint32_t n) {
    uint32_t c0 = 0u, c1 = stream, c2 = t, c3 = SLOT_COND, k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return (uint32_t)mulhi64(((uint64_t)c1 << 32) | c0, (uint64_t)n);
}

// ---- ancestor sampling (opt-in per handle: SMC_FLAG_ANCESTOR_SAMPLING; Lindsten, Jordan and Schoen 2014) ------------
// Particle Gibbs WITHOUT the backward walk.  The steps are the conditional steps above, unchanged.  After the T recorded steps of
// one filter - clouds (x_t, w_t) with w the dense weights, ancestor vectors a_t (a_t[i]: the particle of step t - 1 that particle i
// of step t descends from; the retained slot's entry is k*_{t-1}), the reference xref the steps ran with, the filter seed, the
// filter's stream id and a path seed - the sweep is:
//   THE ANCESTOR DRAW, t = 1 .. T-1: the pinned particle of step t redraws its ancestor given where it sits,
//       P(J_t = l) ~ w_{t-1}^l f(xref[t] | x_{t-1}^l).  It is ONE step of backward simulation over the cloud of step t - 1 with the
//       target xref[t] in the place of x_{t+1}^j: live sources, b_l, M, q_l = path_weight(b_l, M), the integer sum S and "the smallest
//       i with C_i > r" are those of "backward simulation" above, bit for bit; the uniform is
//       u = anc_uniform(filter seed, stream, t) = v[1] << 32 | v[0] of draw(seed, 0, stream, t, SLOT_ANC),  r = mulhi64(u, S).
//       S = 0 (no live source reaches xref[t]): J_t = k*_{t-1} = cond_slot(seed, stream, t - 1, n), the ancestor it has without
//       sampling.  J_0 = -1.  Every J_t is a function of the OLD reference and of the record alone, not of another J: the T - 1
//       draws are independent given the clouds, which is why the device makes them in one launch.
//   THE LAST INDEX: idx[T-1] is backward simulation's last step for path 0 under the path seed: b_l = sp_log(w_{T-1}^l),
//       u = path_uniform(path_seed, 0, stream, T - 1).  S = 0 there (the last cloud has no live particle): the filter is DEAD,
//       idx[t] = -1 for every t, and it keeps its reference.
//   THE TRACE, t = T-1 .. 1:  idx[t-1] = anc_trace: J_t when idx[t] is the retained slot k*_t, else a_t[idx[t]].
//   THE NEW REFERENCE: xref[t] = x_t^{idx[t]}, copied bit for bit, after every J_t has been drawn from the old one.
// The kernel on trajectories leaves p(x_1:T | y_1:T, theta) invariant for any n >= 2, as backward simulation does.
constexpr uint32_t SLOT_ANC = 39u;   // no other draw uses it (the other slots end at 38)
// v[1] << 32 | v[0] of draw(seed, 0, stream, t, slot) by plain integer operators: the loop of cond_slot (which is left as it
// is, so that the step kernels compile from unchanged text), for a draw that is uniform over a workgroup and wants the scalar unit
SMC_HD uint64_t scalar_draw64(uint64_t seed, uint32_t stream, uint32_t t, uint32_t slot) {
    uint32_t c0 = 0u, c1 = stream, c2 = t, c3 = slot, k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return ((uint64_t)c1 << 32) | c0;
}
SMC_HD uint64_t anc_uniform(uint64_t seed, uint32_t stream, uint32_t t) { return scalar_draw64(seed, stream, t, SLOT_ANC); }
// one step of the trace: the particle of step t - 1 behind particle i of step t (kstar = k*_t, J = J_t, a_t the ancestors of step t)
SMC_HD int32_t anc_trace(int32_t i, uint32_t kstar, int32_t J, const int32_t* a_t) { return (uint32_t)i == kstar ? J : a_t[i]; }

// ---- predictive checks: PIT and one-step forecast moments ------------------------------------------------------------
// A bootstrap filter resamples at every step, so the cloud x_t a step leaves, taken WITHOUT its weights, is a sample of
// p(x_t | y_1:t-1); pushed through the observation law it is the predictive law of y_t.  The row of one cloud - one filter at one
// step, n particles in the order of smc_get_state, the observation y, the filter's parameter row - is, with
// (ym_i, sd_i) = model_obs_moments(x_i) and z_i = model_obs_z(x_i, y):
//     pit      = pred_sum(Phi(z_i)) / n                                             P(Y_t <= y_t | y_1:t-1), uniform under the model
//     obs_mean = pred_sum(ym_i) / n
//     obs_var  = pred_sum(sd_i * sd_i) / n + pred_sum((ym_i - obs_mean)^2) / n      a centred second pass
// Phi = sp_normcdf, the four divisions are divisions by (double)n.  A pure function of (cloud, y, row): no weight is read and there
// is no rule for non-finite values, gaps or dead filters - a NaN y gives a NaN pit beside ordinary moments (the forecast of the
// unobserved y_t), an infinite y gives 0 or 1, a NaN state or a zero sd does what IEEE arithmetic does with it.
//
// sp_normcdf(z): with a = |z|, the upper tail is Q(a) = exp(-a^2 / 2) H(s), t = 1 / (1 + a / 4), s = (t - tc) / th in [-1, 1] for
// a in [0, 9]; H = Mills' ratio / sqrt(2 pi) is smooth there and is a polynomial of degree 20 in s (Chebyshev interpolation, monomial
// basis: every coefficient is below 1, Horner's rule by fma; scripts/dbg/normcdf_coeffs.py derives them with mpmath - the
// polynomial itself is within 2.5e-19 of Q before any rounding).  Beyond a = 9 the argument of H stays at 9: Q(9) = 1.13e-19 bounds
// that.  Phi(z) = Q(a) for z <= 0 and 1 - Q(a) for z > 0.  One division, one sp_exp, 23 fma, the same on every input; the pieces
// join at 0 and at +-9.  Phi(-inf) = +0 and Phi(+inf) = 1 (sp_exp(-inf) = 0), a NaN comes back as it is, 0 <= Phi <= 1 always
// (H > 0 and Q <= 1/2 + 1 ulp).  The error of exp's argument, at most half an ulp of a^2 / 2, is a RELATIVE error of Q: the
// absolute one, a^2 Q(a) 2^-54, stays below 1e-17.
// Measured against mpmath at 50 digits (tests/test_predictive_host.py: 200001 points of [-40, 40], the joints +-4 ulp, zeros,
// subnormals, infinities): the largest absolute error is SP_NORMCDF_MAX_ERR below; the contract is 1e-15.
constexpr double SP_NORMCDF_MAX_ERR = 1.9e-16;   // measured 1.886e-16, at z = 0.326; the test reads this line and asserts its maximum against it
constexpr double NORMCDF_AMAX = 9.0;
SMC_HD double sp_normcdf(double z) {
    const double a = fabs(z);
    const double ac = a < NORMCDF_AMAX ? a : NORMCDF_AMAX;   // (a NaN takes 9 here and leaves as itself below)
    const double t = 1.0 / fma(0.25, ac, 1.0);
    const double s = fma(t, 0x1.71c71c71c71c7p+1, -0x1.e38e38e38e38ep+0);
    double h = 0x1.3af85338f8637p-41;
    h = SMC_FMAK(h, s, 0x1.131eff9b8a2b4p-39);
    h = SMC_FMAK(h, s, -0x1.08eabef25d6c5p-36);
    h = SMC_FMAK(h, s, -0x1.5e7f01a3559d1p-38);
    h = SMC_FMAK(h, s, 0x1.de094d2cf7ec5p-33);
    h = SMC_FMAK(h, s, -0x1.b47ca97ef9893p-32);
    h = SMC_FMAK(h, s, -0x1.3025dd8fb5a73p-29);
    h = SMC_FMAK(h, s, 0x1.5a6dd0975dde9p-27);
    h = SMC_FMAK(h, s, 0x1.19ea251311c6dp-26);
    h = SMC_FMAK(h, s, -0x1.89c33ebb25cc7p-23);
    h = SMC_FMAK(h, s, -0x1.55802782421a1p-24);
    h = SMC_FMAK(h, s, 0x1.b8f0cdb045c3dp-19);
    h = SMC_FMAK(h, s, 0x1.5250a97f051dbp-20);
    h = SMC_FMAK(h, s, -0x1.14bc83178dfaap-14);
    h = SMC_FMAK(h, s, -0x1.16e937f7e563ep-13);
    h = SMC_FMAK(h, s, 0x1.4a4a7780eb264p-10);
    h = SMC_FMAK(h, s, 0x1.4a781132135a3p-7);
    h = SMC_FMAK(h, s, 0x1.4038f25527432p-5);
    h = SMC_FMAK(h, s, 0x1.9d73e8b76d46fp-4);
    h = SMC_FMAK(h, s, 0x1.80a48d7396201p-3);
    h = SMC_FMAK(h, s, 0x1.49bd3b6b47470p-3);
    const double q = sp_exp(-0.5 * (a * a)) * h;
    const double r = z > 0.0 ? 1.0 - q : q;
    return z != z ? z : r;
}

// the standardised residual of y under the observation law at x, exactly as model_logobs forms it
template <int MODEL>
SMC_HD double model_obs_z(const Params& p, const double* x, double y) {
    if constexpr (MODEL == MODEL_LG1D) return (y - p.raw[1] * x[0]) * p.der[3];
    else if constexpr (MODEL == MODEL_SV1D) return y * sp_exp(-0.5 * x[0]);
    else return (y - x[0]) * sp_exp(-0.5 * x[2]);
}
// the state rows the predictive row of a family reads: row 0, and for UCSV3D row 2 (the log-variance of the observation noise)
template <int MODEL> struct pred_rows { static constexpr int count = MODEL == MODEL_UCSV3D ? 2 : 1, second = 2; };
// the three terms of the first pass for one particle (x: the rows of pred_rows in their places, the others are not read)
template <int MODEL>
SMC_HD void pred_terms(const Params& p, const double* x, double y, double& cdf, double& ym, double& s2) {
    double sd;
    model_obs_moments<MODEL>(p, x, ym, sd);
    s2 = sd * sd;
    cdf = sp_normcdf(model_obs_z<MODEL>(p, x, y));
}
SMC_HD double pred_centred_term(double ym, double obs_mean) {
    const double dm = ym - obs_mean;
    return dm * dm;
}
// pred_sum: the smoother's order made recursive.  Level 0 cuts the index into chunks of SMOOTH_CH consecutive terms and sums each in
// ascending order with plain adds from +0.0; level k sums SMOOTH_CH consecutive partials of level k - 1 in the same way, until one
// number is left.  For n <= SMOOTH_CH^2 it is smooth_sum bit for bit; no serial run is longer than SMOOTH_CH, whatever n.
// pred_level: one level, m_in numbers to ceil(m_in / SMOOTH_CH) (in place is fine: entry j is written after its chunk was read)
inline int64_t pred_level(const double* in, int64_t m_in, double* out) {
    const int64_t m_out = (m_in + SMOOTH_CH - 1) / SMOOTH_CH;
    for (int64_t j = 0; j < m_out; ++j) {
        double s = 0.0;
        const int64_t c1 = (j + 1) * SMOOTH_CH < m_in ? (j + 1) * SMOOTH_CH : m_in;
        for (int64_t i = j * SMOOTH_CH; i < c1; ++i) s += in[i];
        out[j] = s;
    }
    return m_out;
}
// host only; part: scratch of ceil(n / SMOOTH_CH) doubles
template <class F>
inline double pred_sum(int64_t n, F term, double* part) {
    int64_t m = (n + SMOOTH_CH - 1) / SMOOTH_CH;
    for (int64_t j = 0; j < m; ++j) {
        double s = 0.0;
        const int64_t c1 = (j + 1) * SMOOTH_CH < n ? (j + 1) * SMOOTH_CH : n;
        for (int64_t i = j * SMOOTH_CH; i < c1; ++i) s += term(i);
        part[j] = s;
    }
    while (m > 1) m = pred_level(part, m, part);
    return part[0];
}
// the row from its four sums
SMC_HD double pred_mean_of(double sum, int64_t n) { return sum / (double)n; }
SMC_HD double pred_var_of(double sum_s2, double sum_c, int64_t n) { return sum_s2 / (double)n + sum_c / (double)n; }

// The exact Kalman row, beside kalman_step_gaps: the predictive law of y_t from the predicted pair (x-, S-) as kalman_step forms it
// (at the first step of a filter with predict_first = 0 the pair is (x0, sigma0)), then the step itself.
//     ym = B x-,   yv = (B B) S- + R  (the step's own innovation variance),   z = (y - ym) / sqrt(yv),   pit = sp_normcdf(z)
// At a gap (MISS and a NaN y) the row is (NaN, ym, yv): z is NaN and sp_normcdf hands it back.  (x, S) are advanced in place by
// kalman_step_gaps from the values they had: the filter's bits are those of a run that never asked.
template <bool MISS>
SMC_HD void kalman_predictive_step(double A, double B, double Q, double R, bool predict, double y, double& x, double& S, double& pit, double& ym,
                                   double& yv) {
    const double xm = predict ? A * x : x, Sm = predict ? (A * A) * S + Q : S;
    ym = B * xm;
    yv = (B * B) * Sm + R;
    pit = sp_normcdf((y - ym) / sqrt(yv));
    (void)kalman_step_gaps<MISS>(A, B, Q, R, predict, y, x, S);
}

}  // namespace smc
