// OSD post-processing (DESIGN.md sections 1.2 and 1.3: OSD-0 and the combination sweep OSD-CS): the
// per-sector tables both implementations read, the host implementation (osd_host.cpp) and the kernel
// launchers (osd.hip).
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "qec_internal.h"

namespace qec {

// One sector's parity-check matrix for the elimination.
struct OsdSector {
    int m = 0, n = 0;
    int W = 0;                   // 32-bit words per row of the augmented matrix [H | s]: ceil((n + 1) / 32)
    int rank = 0;                // rank(H) over GF(2): the column walk stops there
    std::vector<uint32_t> H;     // m x W, bit v of row c = H[c][v] (bit v % 32 of word v / 32); column n clear
    std::vector<int32_t> qpos;   // n: offset, in one sample's q_final block, of the slot of v at the lowest-index
                                 // check that contains v; -1 if no check does (key 0.5 then)
};

struct OsdPlan {
    OsdSector sec[2];
    size_t qn = 0;  // floats of one sample's q_final block: (mX + mZ) L
};

// Sort key of a soft value: NaN -> the pattern of 0.5f, else the sign bit cleared;
// keys compare as unsigned integers.
constexpr uint32_t kOsdHalf = 0x3F000000u;
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t osd_key(uint32_t bits)
{
    const uint32_t a = bits & 0x7FFFFFFFu;
    return a > 0x7F800000u ? kOsdHalf : a;
}

// Sort key of a soft value that is an LLR (QEC_OPT_BP_METHOD = 1: q_final holds LLRs, > 0 = the bit is 0): the
// column order runs by LLR ascending, so the key is the complement of the usual order-preserving map of a float's
// pattern onto unsigned integers.  -0.0f sorts directly before +0.0f; every LLR is finite.  The key of a variable in
// no check is that of +0.0f.
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t osd_key_llr(uint32_t bits)
{
    return ~(bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u));
}
constexpr uint32_t kOsdLlrZero = 0x7FFFFFFFu;  // osd_key_llr of +0.0f

void osd_plan_build(const Code& c, OsdPlan& out);

constexpr int kOsdMaxOrder = 64;  // QEC_OPT_OSD_ORDER: lambda of the combination sweep, 0 .. 64

// QEC_OPT_OSD_SCORE = 1: the sweep's integer weight of a flip on a qubit of prior pi, in
// sixteenths of a bit of log-likelihood ratio: 0 for pi >= 1/2, 4095 for pi = 0, else
// min(4095, llrint(16 log2((1 - pi) / pi))), the float taken exactly to double.
constexpr int kOsdMaxWeight = 4095;
int32_t osd_weight(float prior);

// Steps 2-6 for one sector of one sample: q = the sample's q_final block, s = the sector's syndrome
// bytes, e = the sector's estimate (n bytes), rewritten only if [H | s] is consistent.  Returns
// whether it was.  order = lambda of section 1.3 (0: the OSD-0 estimate); *swept (nullable) tells
// whether the lightest candidate was another than the OSD-0 estimate (index > 0).  w (nullable): the
// sector's n weights of section 1.4; the candidate of least score wins instead of the lightest.
// llr: q holds LLRs (osd_key_llr) instead of probabilities (osd_key); everything behind the key is the same.
bool osd_host_sector(const OsdSector& S, const float* q, const uint8_t* s, uint8_t* e, int order = 0,
                     bool* swept = nullptr, const int32_t* w = nullptr, bool llr = false);

// Steps 2-7 on a decoded host batch, in place; returns the number of sectors repaired, and in
// *swept (nullable) how many of them took a candidate of index > 0.  w (nullable): the weight tables
// of section 1.4, sector X [n] then sector Z [n].
long long osd_host_batch(const OsdPlan& P, const uint8_t* sX, const uint8_t* sZ, long long B, const float* q,
                         uint8_t* eX, uint8_t* eZ, uint8_t* flags, int threads, int order = 0,
                         long long* swept = nullptr, const int32_t* w = nullptr, bool llr = false);

}  // namespace qec
