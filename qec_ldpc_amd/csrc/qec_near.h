// The near-hard jump's threshold (QEC_OPT_NEAR_HARD_JUMP), shared by the
// wave-circulant kernels' launch (bp_decode.hip) and the CPU engine (cpu_engine.cpp).
//
// A sector's state after a var pass satisfies C(eps0) when some assignment h with H h = s has every
// variable->check message of variable v in [0, eps0] (h_v = 0) or in [1 - eps0, 1] (h_v = 1).  With
//   delta = (L - 1) eps0 + 2^-20   and   2 ((1 - p') / p') (delta / (1 - delta))^(R - 1) <= eps0
// C(eps0) is kept by every later iteration in the decoder's own fp32 operations (the lemma of DESIGN.md
// 4.1 item 15), so the decisions (h), both flags (clear) and the iteration count of a fixed- or
// reference-stop decode are known the moment it holds.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

namespace qec {

struct NearHard {
    float eps0;   // 0: the jump never fires; else a power of two in [2^-20, 2^-8]
    uint32_t T;   // compare value: bits(fma(-q, q, q)) <= T (unsigned) implies q <= eps0 or q >= 1 - eps0
};

// eps0: the largest power of two in [2^-20, 2^-8] that satisfies the inequality above for p' (the float
// the decoder forms), R checks per variable and L variables per check, evaluated in double; none, or
// p' outside (0, 1/2] (the lemma's h = 0 side needs p' / (1 - p') <= (1 - p') / p'), or L > 32 (the
// rounding terms of an (L - 1)-fold product are bounded by 2^-20 up to there): {0, 0}.
// T: q (1 - q) rises on [0, 1/2] and falls on [1/2, 1] and rounding is monotone, so a q in
// (eps0, 1 - eps0) has RN(q - q q) >= eps0 (1 - eps0), which is a float (eps0 a power of two >= 2^-20);
// T is the bit pattern one below it.  A NaN or a negative value compares above every such T.
inline NearHard near_hard_threshold(float pp, int R, int L)
{
    NearHard out{0.0f, 0u};
    if (!(pp > 0.0f && pp <= 0.5f) || R < 2 || L < 2 || L > 32) return out;
    const double odds = (1.0 - (double)pp) / (double)pp;
    for (int k = 8; k <= 20; ++k) {
        const double e = std::ldexp(1.0, -k);
        const double d = (L - 1) * e + 0x1p-20;
        if (!(d < 0.5)) continue;
        const double ratio = d / (1.0 - d);
        double x = 2.0 * odds;
        for (int f = 0; f < R - 1; ++f) x *= ratio;
        // a relative 2^-40 of slack: whoever re-evaluates the inequality in another order of double
        // operations finds it satisfied too
        if (!(x * (1.0 + 0x1p-40) <= e)) continue;
        out.eps0 = (float)e;
        const float v = (float)(e - e * e);  // exact: k <= 20 significand bits
        std::memcpy(&out.T, &v, sizeof v);
        out.T -= 1u;
        return out;
    }
    return out;
}

// The near-hard probe (QEC_OPT_NEAR_PROBE): the var-view half of C(eps0) read from the
// two folds t0, t1 of an outgoing message q = t1 / (t0 + t1) before any division is made.
//
// On the bit patterns b0, b1 of t0, t1: both below 0x7F000000 (non-negative -- -0 excluded --, finite, below
// 2^127, no NaN) and |b1 - b0| >= K with K = near_probe_scale(eps0) = (k + 1) << 23 for eps0 = 2^-k.  For
// non-negative floats the map b -> value is monotone and value(b + 2^23) >= 2 value(b) (equality for normal b;
// a subnormal or zero b lands in the first normal binade, at value (2^23 + b) 2^-149 >= 2 b 2^-149), so
// |b1 - b0| >= K implies max(t0, t1) >= (2 / eps0) min(t0, t1), max(t0, t1) > 0: the integer test is the
// ratio test, exact on normal folds and stricter below them; two zeros fail (K > 0).
//
// Then q' = RN(t1 / RN(t0 + t1)) -- what the IEEE and the short division both return, for the 2^32-scaled
// folds too (the same quotient) -- satisfies, with u = 2^-24 and RN monotone:
//   t1 (2 / eps0) <= t0:  RN(t0 + t1) >= t0, so q' <= RN(t1 / t0) <= eps0 / 2, and
//                         RN(q' - q' q') <= q' <= eps0 / 2 < eps0 (1 - eps0);
//   t0 (2 / eps0) <= t1:  t1 <= RN(t0 + t1) <= t1 (1 + eps0 / 2)(1 + u) (the sum is normal and below 2^128), so
//                         1 >= q' >= 1 - eps0 / 2 - 2 u >= 1 - (5 / 8) eps0 (eps0 >= 2^-20 = 16 u), and
//                         RN(q' - q' q') <= RN(1 - q') <= (5 / 8) eps0 < eps0 (1 - eps0) (eps0 <= 2^-8).
// In both cases fma(-q', q', q') is non-negative and its bits are <= T of near_hard_threshold, and
// q' >= 0.5f exactly when t1 > t0: a probe that passes is a state var_pass's exact test passes, with the same
// sides.  The fold length does not enter (any t0, t1 of that domain).
inline uint32_t near_probe_scale(float eps0)
{
    int e = 0;
    if (!(eps0 > 0.0f) || std::frexp(eps0, &e) != 0.5f) return 0u;  // eps0 = 2^(e - 1)
    const int k = 1 - e;
    return k >= 8 && k <= 20 ? (uint32_t)(k + 1) << 23 : 0u;
}
constexpr uint32_t kNearProbeTop = 0x7F000000u;  // every fold's bit pattern lies below it
// One variable's R outputs, one at a time (NearProbeVar::add, the bit patterns of an output's folds), then the
// largest K they pass on one common side of 0.5 (margin; <= 0 if none): min_j (b1_j - b0_j) when every output lies
// above (side = 1), min_j (b0_j - b1_j) when below (side = 0) -- valid when top, which accumulates the unsigned
// maximum of every pattern seen, stays below kNearProbeTop.  The variable passes iff margin >= K > 0 and
// top < kNearProbeTop; the kernel keeps the minimum margin and the one top of a lane's variables and compares
// once per ballot.
#if defined(__HIPCC__)
#define QEC_NEAR_HD __host__ __device__ __forceinline__
#else
#define QEC_NEAR_HD inline
#endif
struct NearProbeVar {
    int32_t mn = 0x7FFFFFFF, mx = -0x7FFFFFFF - 1;  // extremes of b1_j - b0_j
    QEC_NEAR_HD void add(uint32_t b0, uint32_t b1, uint32_t& top)
    {
        const int32_t d = (int32_t)(b1 - b0);
        mn = d < mn ? d : mn;
        mx = d > mx ? d : mx;
        top = top > b0 ? top : b0;
        top = top > b1 ? top : b1;
    }
    QEC_NEAR_HD int32_t margin() const
    {
        const int32_t neg = (int32_t)(0u - (uint32_t)mx);
        return mn > neg ? mn : neg;
    }
    QEC_NEAR_HD bool side() const { return mn > 0; }
};
#undef QEC_NEAR_HD
// One output.  side (out, when true): 1 iff t1 > t0, the side of 0.5 q' lies on.  eps0 not a power of two in
// [2^-20, 2^-8]: false.
inline bool near_probe(float t0, float t1, float eps0, int& side)
{
    uint32_t b0, b1, top = 0u;
    std::memcpy(&b0, &t0, sizeof t0);
    std::memcpy(&b1, &t1, sizeof t1);
    const uint32_t K = near_probe_scale(eps0);
    NearProbeVar v;
    v.add(b0, b1, top);
    side = v.side();
    return K != 0u && top < kNearProbeTop && v.margin() >= (int32_t)K;
}

}  // namespace qec
