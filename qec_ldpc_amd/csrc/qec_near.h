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

}  // namespace qec
