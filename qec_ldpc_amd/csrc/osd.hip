// OSD post-processing on the device (DESIGN.md sections 1.2, 1.3, section 6): one wave64 per failed
// sector eliminates the bit-packed augmented matrix [H | s] in LDS, walking the columns in the order of
// the soft input; with QEC_OPT_OSD_ORDER > 0 the same wave then scores the combination sweep on the
// reduced matrix.  Beside it the three small kernels of the Monte-Carlo path (failed-record list, syndrome
// gather, write-back into the packed decision records).  gfx950 only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "qec_device.h"
#include "qec_osd.h"

namespace qec {

// Device copy of an OsdPlan (tables uploaded by osd_dev_create).
struct OsdDev {
    const uint32_t* H[2];     // m x W bit rows
    const int32_t* qpos[2];   // n offsets into a sample's q_final block (-1: none)
    int m[2];
    int rank[2];
    int n;
    int W;                    // words per row: ceil((n + 1) / 32)
    int Ws;                   // LDS row stride in words: W padded to an odd count, so lanes that each read a
                              // row of their own (the pivot search) fall on 32 distinct banks per half-wave
    long long qn;             // floats of one sample's q_final block
    int sweep;                // QEC_OPT_OSD_SWEEP: how a pivot row is XORed into the rows with the bit
};

// What the sweep takes beside it (behind the arguments the order-0 kernel always had).
struct OsdCs {
    int order;                // QEC_OPT_OSD_ORDER: lambda of the combination sweep
    int RWs;                  // LDS stride in words of a column's bit vector over the rows (odd, see osd_rws)
};

struct OsdDevPlan {
    OsdDev d{};
    void* mem = nullptr;      // one allocation behind the four tables
    uint32_t lds_bytes = 0;
    int mmax = 0;
};

namespace {

constexpr uint32_t kOsdMaxLds = 64u * 1024u;  // one workgroup's dynamic LDS allocation
constexpr int kOsdMaxN = 2048;                // the logical check's limit; rows: 32 chunks of 64 (the used-row mask)

int launch_check(const char* what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(QEC_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    return QEC_OK;
}

// Words of a bit vector over the rows, one 64-bit ballot per chunk of 64 rows, padded to an odd count
// so that lanes reading a vector each (the pairs) spread over the banks.
__host__ __device__ inline int osd_rws(int mmax) { return (2 * ((mmax + 63) >> 6)) | 1; }

// LDS image of one wave (32-bit words): rows [mmax][Ws] | keys [n] (later the estimate's bytes [n]
// and, for the sweep, T [n] u16 behind them: ceil(n / 4) + ceil(n / 2) <= n words for n >= 2) |
// order [n] u16 | pivcol [mmax] u16 | for lambda > 0 the bit vectors of the first lambda columns of T
// and of s': [lambda + 1][RWs] | for the weighted sweep (section 1.4) the bit-planes of the rows'
// weights [kOsdPlanes][RWs] and the weights themselves, wp [mmax] u16
constexpr int kOsdPlanes = 12;  // bits of a weight (kOsdMaxWeight = 4095)
__host__ __device__ inline uint32_t osd_lds_words(int mmax, int n, int Ws, int order, bool weighted = false)
{
    return (uint32_t)mmax * Ws + n + (n + 1) / 2 + (mmax + 1) / 2 +
           (order > 0 ? (uint32_t)(order + 1) * osd_rws(mmax) : 0u) +
           (order > 0 && weighted ? (uint32_t)kOsdPlanes * osd_rws(mmax) + (mmax + 1) / 2 : 0u);
}

// Block t: sample t / 2, sector t % 2.  A sector without its SYNDROME_FAIL bit exits at once, so the
// launch needs no list of failures.  Writes: e[b][0, n) and the sector's bit of flags[b], both only
// when [H | s] is consistent; *repaired (nullable) counts those sectors.  CS: the combination sweep
// of section 1.3 between the consistency test and the write-out; *swept (nullable) counts the sectors
// whose lightest candidate is not the OSD-0 estimate.
// The kernel itself is the template (osd_kernel<false> is the order-0 kernel, instruction for
// instruction what it was before the sweep existed: a shared body inlined into two kernels compiled
// to a slower elimination loop).  WEIGHTED (with CS): the sweep scores a candidate by the sum of
// wt[v] over its flips (section 1.4; wt = the two sectors' tables, [2][n]) instead of their number;
// the other two instantiations never read wt.  LLR (QEC_OPT_BP_METHOD = 1): q holds LLRs and the keys are
// osd_key_llr's; a template parameter, so the instantiations without it keep their instruction streams.
template <bool CS, bool WEIGHTED = false, bool LLR = false>
__global__ __launch_bounds__(64) void osd_kernel(OsdDev P, const uint8_t* __restrict__ sX,
                                                 const uint8_t* __restrict__ sZ, long long B,
                                                 const float* __restrict__ q, uint8_t* __restrict__ eX,
                                                 uint8_t* __restrict__ eZ, uint8_t* flags, uint32_t* repaired,
                                                 OsdCs C, uint32_t* swept, const int32_t* __restrict__ wt)
{
    static_assert(CS || !WEIGHTED, "the weighted score belongs to the sweep");
    extern __shared__ uint32_t lds[];
    const long long b = (long long)(blockIdx.x >> 1);
    const int sec = (int)(blockIdx.x & 1u);
    if (b >= B) return;
    const uint32_t fbit = sec ? QEC_SYNDROME_FAIL_Z : QEC_SYNDROME_FAIL_X;
    if (!(flags[b] & fbit)) return;

    const int lane = (int)threadIdx.x;
    const int m = P.m[sec], n = P.n, W = P.W, Ws = P.Ws, rank = P.rank[sec];
    const int mmax = P.m[0] > P.m[1] ? P.m[0] : P.m[1];
    uint32_t* rows = lds;
    uint32_t* keys = rows + (size_t)mmax * Ws;
    uint16_t* order = reinterpret_cast<uint16_t*>(keys + n);
    uint16_t* pivcol = order + 2 * ((n + 1) / 2);
    const uint32_t* H = P.H[sec];
    const int32_t* qpos = P.qpos[sec];
    const uint8_t* s = (sec ? sZ : sX) + b * m;
    const float* qb = q + b * P.qn;
    uint8_t* e = (sec ? eZ : eX) + b * n;
    const int sw = n >> 5;
    const uint32_t sbit = 1u << (n & 31);
    const int nchunk = (m + 63) >> 6;

    // [H | s] into LDS
    for (int i = lane; i < m * W; i += 64) {
        const int r = i / W;
        rows[r * Ws + (i - r * W)] = H[i];
    }
    wave_sync();
    bool bad = false;  // an entry other than 0 or 1 is never reproduced
    for (int c = lane; c < m; c += 64) {
        const uint8_t sv = s[c];
        bad |= sv > 1;
        if (sv == 1) rows[c * Ws + sw] |= sbit;
    }
    if (__ballot(bad)) return;
    // keys, then each column's rank by counting: #{u : key(u) > key(v) or (key(u) = key(v) and u < v)}
    for (int v = lane; v < n; v += 64) {
        const int p = qpos[v];
        if (LLR) keys[v] = p < 0 ? kOsdLlrZero : osd_key_llr(__float_as_uint(qb[p]));
        else keys[v] = p < 0 ? kOsdHalf : osd_key(__float_as_uint(qb[p]));
    }
    wave_sync();
    for (int v = lane; v < n; v += 64) {
        const uint32_t kv = keys[v];
        int r = 0;
        for (int u = 0; u < n; ++u) {
            const uint32_t ku = keys[u];  // one address per wave: a broadcast
            r += (ku > kv) || (ku == kv && u < v);
        }
        order[r] = (uint16_t)v;
    }
    wave_sync();

    // Gauss-Jordan over the columns in that order.  Lane l owns rows l, l + 64, ...: bit k of `used`
    // marks row 64 k + l as a pivot row.
    uint32_t used = 0;
    int npiv = 0;
    for (int t = 0; t < n && npiv < rank; ++t) {
        const int v = order[t];
        const int w = v >> 5;
        const uint32_t bit = 1u << (v & 31);
        // the lowest unused row with the bit: a ballot per chunk of 64 rows
        int prow = -1;
        for (int k = 0; k < nchunk && prow < 0; ++k) {
            const int r = (k << 6) + lane;
            const bool cand = r < m && !((used >> k) & 1u) && (rows[r * Ws + w] & bit);
            const unsigned long long bal = __ballot(cand);
            if (bal) prow = (k << 6) + __ffsll((long long)bal) - 1;
        }
        if (prow < 0) continue;  // dependent on the pivots chosen so far
        // XOR the pivot row into every other row with the bit, a chunk of 64 rows at a time.  Two forms:
        //   words: lanes across the W words, a wave-uniform loop over the rows a ballot found (no
        //          divergence, min(W, 64) lanes busy; popcount x ceil(W / 64) steps);
        //   rows:  every lane whose own row has the bit walks its W words (the odd row stride keeps the
        //          lanes on distinct banks, the pivot row's word is a broadcast; W steps).
        // QEC_OPT_OSD_SWEEP = 0 takes per chunk the form with fewer steps: early columns meet a few
        // rows (the column weight), late ones about half of them.
        const uint32_t* pr = rows + prow * Ws;
        for (int k = 0; k < nchunk; ++k) {
            const int r = (k << 6) + lane;
            const bool has = r < m && r != prow && (rows[r * Ws + w] & bit);
            unsigned long long bal = __ballot(has);
            const bool by_rows = P.sweep == 2 || (P.sweep == 0 && __popcll(bal) * ((W + 63) >> 6) > W);
            if (by_rows) {
                if (has)
                    for (int x = 0; x < W; ++x) rows[r * Ws + x] ^= pr[x];
            } else {
                while (bal) {
                    const int rr = (k << 6) + __ffsll((long long)bal) - 1;
                    bal &= bal - 1;
                    for (int x = lane; x < W; x += 64) rows[rr * Ws + x] ^= pr[x];
                }
            }
            wave_sync();
        }
        if (lane == (prow & 63)) used |= 1u << (prow >> 6);
        if (lane == 0) pivcol[prow] = (uint16_t)v;
        ++npiv;
    }
    wave_sync();
    // rows without a pivot are zero in H now; s is in the column space iff they are zero in s too
    bool incons = false;
    for (int k = 0; k < nchunk; ++k) {
        const int r = (k << 6) + lane;
        incons |= r < m && !((used >> k) & 1u) && (rows[r * Ws + sw] & sbit);
    }
    if (__ballot(incons)) return;
    uint8_t* eb = reinterpret_cast<uint8_t*>(keys);
    int fa = -1, fb = -1;  // CS: the columns the lightest candidate flips (wave-uniform)
    if constexpr (CS) {
        // T = the non-pivot columns in the walk's order, behind the estimate's bytes: mark the pivot
        // columns in those bytes, then compact `order` a ballot of 64 entries at a time
        uint16_t* T = reinterpret_cast<uint16_t*>(keys + (n + 3) / 4);
        for (int v = lane; v < n; v += 64) eb[v] = 0;
        wave_sync();
        for (int k = 0; k < nchunk; ++k) {
            const int r = (k << 6) + lane;
            if (r < m && ((used >> k) & 1u)) eb[pivcol[r]] = 1;
        }
        wave_sync();
        int f = 0;
        for (int t0 = 0; t0 < n; t0 += 64) {
            const int t = t0 + lane;
            const int v = t < n ? order[t] : 0;
            const bool free = t < n && !eb[v];
            const unsigned long long bal = __ballot(free);
            if (free) T[f + __popcll(bal & ((1ull << lane) - 1ull))] = (uint16_t)v;
            f += __popcll(bal);
        }
        wave_sync();
        // bit vectors over the rows (bit r of word pair k = row 64 k + r; rows without a pivot are zero):
        // s' and the first lam columns of T; |s'| is the OSD-0 estimate's weight
        const int lam = C.order < f ? C.order : f;
        const int RWs = C.RWs, RW = 2 * nchunk;
        uint32_t* cv = reinterpret_cast<uint32_t*>(pivcol + 2 * ((mmax + 1) / 2));
        uint32_t* sv = cv + lam * RWs;
        int w0 = 0;
        for (int k = 0; k < nchunk; ++k) {
            const int r = (k << 6) + lane;
            const unsigned long long bal = __ballot(r < m && (rows[r * Ws + sw] & sbit));
            w0 += __popcll(bal);
            if (lane < 2) sv[2 * k + lane] = (uint32_t)(bal >> (32 * lane));
        }
        for (int j = 0; j < lam; ++j) {
            const int v = T[j];  // one address per wave: a broadcast
            const int w = v >> 5;
            const uint32_t bit = 1u << (v & 31);
            for (int k = 0; k < nchunk; ++k) {
                const int r = (k << 6) + lane;
                const unsigned long long bal = __ballot(r < m && (rows[r * Ws + w] & bit));
                if (lane < 2) cv[j * RWs + 2 * k + lane] = (uint32_t)(bal >> (32 * lane));
            }
        }
        wave_sync();
        int idx;
        if constexpr (WEIGHTED) {
            // section 1.4: wp[r] = the weight of row r's pivot column (0 without a pivot), and its bit-planes
            // stored as s' is: plane q holds bit q of every row's weight, so that the weight of a bit vector x
            // over the rows is the sum over q of 2^q popc(x & plane q).  Only the planes up to the highest
            // set bit of any weight are built and read (nq, wave-uniform).
            const int32_t* wsec = wt + (size_t)sec * n;
            uint32_t* pl = sv + RWs;
            uint16_t* wp = reinterpret_cast<uint16_t*>(pl + kOsdPlanes * RWs);
            uint32_t s0 = 0, wor = 0;  // this lane's share of the OSD-0 estimate's score; OR of its rows' weights
            for (int k = 0; k < nchunk; ++k) {
                const int r = (k << 6) + lane;
                const bool piv = r < m && ((used >> k) & 1u);
                const uint32_t wr = piv ? (uint32_t)wsec[pivcol[r]] : 0u;
                if (r < m) wp[r] = (uint16_t)wr;
                if (piv && (rows[r * Ws + sw] & sbit)) s0 += wr;
                wor |= wr;
                for (int q = 0; q < kOsdPlanes; ++q) {
                    const unsigned long long bal = __ballot((wr >> q) & 1u);
                    if (lane < 2) pl[q * RWs + 2 * k + lane] = (uint32_t)(bal >> (32 * lane));
                }
            }
            for (int o = 32; o; o >>= 1) {
                s0 += (uint32_t)__shfl_xor((int)s0, o);
                wor |= (uint32_t)__shfl_xor((int)wor, o);
            }
            const int nq = 32 - __clz(wor);  // __clz(0) = 32: no plane at all
            wave_sync();
            // (score, index) keys: scores <= (rank + 2) 4095 < 2^23, indices < 2^12
            unsigned long long best = (unsigned long long)s0 << 12;
            // singles: flipping t adds its own weight, and wp[r] for each row with R[r][t] = 1 and s'[r] = 0,
            // and takes wp[r] away for each with s'[r] = 1
            for (int j0 = 0; j0 < f; j0 += 64) {
                const int j = j0 + lane;
                const int v = j < f ? T[j] : 0;
                const int w = v >> 5, sh = v & 31;
                int d = 0;
                for (int x = 0; x < RW; ++x) {
                    const uint32_t sword = sv[x];  // a broadcast
                    const int r0 = x << 5;
                    const int r1 = r0 + 32 < m ? r0 + 32 : m;
                    for (int r = r0; r < r1; ++r) {
                        const int cb = (int)((rows[r * Ws + w] >> sh) & 1u);
                        const int wr = (int)wp[r];  // a broadcast
                        d += cb * (((sword >> (r - r0)) & 1u) ? -wr : wr);
                    }
                }
                if (j < f) {
                    const unsigned long long c =
                        ((unsigned long long)(uint32_t)((int)s0 + wsec[v] + d) << 12) | (unsigned long long)(1 + j);
                    best = c < best ? c : best;
                }
            }
            // pairs, as below, the popcount taken plane by plane.  w[t_i] and w[t_j] come from the table in
            // global memory (232 B per sector here, cache hits): keeping them in a register per lane and
            // shuffling measured slower inside qec_monte_carlo
            int pidx = 1 + f;
            for (int i = 0; i + 1 < lam; ++i) {
                const int j = i + 1 + lane;
                if (j < lam) {
                    uint32_t sc = (uint32_t)(wsec[T[i]] + wsec[T[j]]);
                    for (int x = 0; x < RW; ++x) {
                        const uint32_t xv = cv[i * RWs + x] ^ sv[x] ^ cv[j * RWs + x];
                        for (int q = 0; q < nq; ++q) sc += (uint32_t)__popc(xv & pl[q * RWs + x]) << q;
                    }
                    const unsigned long long c = ((unsigned long long)sc << 12) | (unsigned long long)(pidx + lane);
                    best = c < best ? c : best;
                }
                pidx += lam - 1 - i;
            }
            for (int o = 32; o; o >>= 1) {
                const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)best, o);
                const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(best >> 32), o);
                const unsigned long long other = ((unsigned long long)hi << 32) | lo;
                best = other < best ? other : best;
            }
            idx = (int)(best & 0xFFFull);
        } else {
            // packed (weight, index): weights <= rank + 2 <= 2050, indices < 1 + 2048 + 2016 < 2^12
            uint32_t best = (uint32_t)w0 << 12;
            // singles, lanes across the columns of T: flipping t changes the weight by one for t itself, by
            // +1 for each row with R[r][t] = 1 and s'[r] = 0, by -1 for each with s'[r] = 1
            for (int j0 = 0; j0 < f; j0 += 64) {
                const int j = j0 + lane;
                const int v = j < f ? T[j] : 0;
                const int w = v >> 5, sh = v & 31;
                int d = 0;
                for (int x = 0; x < RW; ++x) {
                    const uint32_t sword = sv[x];  // a broadcast
                    const int r0 = x << 5;
                    const int r1 = r0 + 32 < m ? r0 + 32 : m;
                    for (int r = r0; r < r1; ++r) {
                        const int cb = (int)((rows[r * Ws + w] >> sh) & 1u);
                        d += cb - 2 * (cb & (int)((sword >> (r - r0)) & 1u));
                    }
                }
                if (j < f) {
                    const uint32_t c = ((uint32_t)(w0 + 1 + d) << 12) | (uint32_t)(1 + j);
                    best = c < best ? c : best;
                }
            }
            // pairs {t_i, t_j}, i < j < lam <= 64: a wave-uniform loop over i, lanes across j
            int pidx = 1 + f;  // index of the pair (i, i + 1)
            for (int i = 0; i + 1 < lam; ++i) {
                const int j = i + 1 + lane;
                if (j < lam) {
                    int wt = 2;
                    for (int x = 0; x < RW; ++x) wt += __popc(cv[i * RWs + x] ^ sv[x] ^ cv[j * RWs + x]);
                    const uint32_t c = ((uint32_t)wt << 12) | (uint32_t)(pidx + lane);
                    best = c < best ? c : best;
                }
                pidx += lam - 1 - i;
            }
            for (int o = 32; o; o >>= 1) {
                const uint32_t other = (uint32_t)__shfl_xor((int)best, o);
                best = other < best ? other : best;
            }
            idx = (int)(best & 0xFFFu);
        }
        if (idx > 0 && idx <= f) {
            fa = T[idx - 1];
        } else if (idx > f) {
            int rem = idx - 1 - f, i = 0;
            while (rem >= lam - 1 - i) {
                rem -= lam - 1 - i;
                ++i;
            }
            fa = T[i];
            fb = T[i + 1 + rem];
        }
        if (lane == 0 && idx > 0 && swept) atomicAdd(swept, 1u);
        wave_sync();
    }
    // the estimate in LDS (over the keys), then out
    for (int v = lane; v < n; v += 64) eb[v] = 0;
    wave_sync();
    for (int k = 0; k < nchunk; ++k) {
        const int r = (k << 6) + lane;
        if constexpr (CS) {
            if (r < m && ((used >> k) & 1u)) {
                uint32_t bit = (rows[r * Ws + sw] & sbit) ? 1u : 0u;
                if (fa >= 0) bit ^= (rows[r * Ws + (fa >> 5)] >> (fa & 31)) & 1u;
                if (fb >= 0) bit ^= (rows[r * Ws + (fb >> 5)] >> (fb & 31)) & 1u;
                eb[pivcol[r]] = (uint8_t)bit;
            }
        } else {
            if (r < m && ((used >> k) & 1u)) eb[pivcol[r]] = (rows[r * Ws + sw] & sbit) ? 1 : 0;
        }
    }
    wave_sync();
    if constexpr (CS) {
        if (lane == 0 && fa >= 0) eb[fa] = 1;
        if (lane == 0 && fb >= 0) eb[fb] = 1;
        wave_sync();
    }
    for (int v = lane; v < n; v += 64) e[v] = eb[v];
    if (lane == 0) {
        // the other sector's wave may clear its own bit of the same byte: an atomic AND on the aligned
        // word that holds the byte (all ones elsewhere, so the neighbouring bytes keep their values)
        const uintptr_t a = reinterpret_cast<uintptr_t>(flags + b);
        atomicAnd(reinterpret_cast<unsigned int*>(a & ~(uintptr_t)3), ~(fbit << (8u * (unsigned)(a & 3))));
        if (repaired) atomicAdd(repaired, 1u);
    }
}

// ---- Monte-Carlo path: packed decision records ------------------------------------------------
// The indices of the records whose flags byte carries a syndrome failure, with an atomic list length.
__global__ void osd_collect_kernel(const uint8_t* __restrict__ rec, int rstride, int fo, long long B,
                                   int32_t* __restrict__ list, uint32_t* count)
{
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    if (rec[b * rstride + fo] & QEC_SYNDROME_FAIL_XZ) list[atomicAdd(count, 1u)] = (int32_t)b;
}

// The listed samples' syndromes (bit rows or bytes) as a compact byte batch, and their flags twice:
// fl for the OSD kernel to update, fl0 for the write-back to compare against.
__global__ void osd_gather_kernel(const int32_t* __restrict__ list, long long cnt, const uint8_t* __restrict__ sX,
                                  const uint8_t* __restrict__ sZ, int bits, int mX, int mZ,
                                  const uint8_t* __restrict__ rec, int rstride, int fo, uint8_t* __restrict__ oX,
                                  uint8_t* __restrict__ oZ, uint8_t* __restrict__ fl, uint8_t* __restrict__ fl0)
{
    const long long i = blockIdx.x;
    if (i >= cnt) return;
    const long long b = list[i];
    const int wX = (mX + 31) / 32, wZ = (mZ + 31) / 32;
    const uint32_t* bX = reinterpret_cast<const uint32_t*>(sX) + b * wX;
    const uint32_t* bZ = reinterpret_cast<const uint32_t*>(sZ) + b * wZ;
    for (int c = (int)threadIdx.x; c < mX; c += (int)blockDim.x)
        oX[i * mX + c] = bits ? (uint8_t)((bX[c >> 5] >> (c & 31)) & 1u) : sX[b * mX + c];
    for (int c = (int)threadIdx.x; c < mZ; c += (int)blockDim.x)
        oZ[i * mZ + c] = bits ? (uint8_t)((bZ[c >> 5] >> (c & 31)) & 1u) : sZ[b * mZ + c];
    if (threadIdx.x == 0) {
        const uint8_t f = rec[b * rstride + fo];
        fl[i] = f;
        fl0[i] = f;
    }
}

// The repaired sectors' estimates and the flags byte back into the records at their own indices
// (record row stride rstride: mc_batch pads rows to whole words on the bit-row path).
__global__ void osd_scatter_kernel(const int32_t* __restrict__ list, long long cnt, const uint8_t* __restrict__ eX,
                                   const uint8_t* __restrict__ eZ, const uint8_t* __restrict__ fl,
                                   const uint8_t* __restrict__ fl0, int n, uint8_t* __restrict__ rec, int rstride)
{
    const int nb = (n + 7) / 8, per = 2 * nb + 1;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= cnt * per) return;
    const long long i = t / per;
    const int k = (int)(t - i * per);
    const uint8_t fixed = fl0[i] & (uint8_t)~fl[i];  // fail bits the OSD stage cleared
    uint8_t* out = rec + (long long)list[i] * rstride;
    if (k == 2 * nb) {
        out[k] = fl[i];
        return;
    }
    const int sec = k >= nb;
    if (!(fixed & (sec ? QEC_SYNDROME_FAIL_Z : QEC_SYNDROME_FAIL_X))) return;
    const uint8_t* e = (sec ? eZ : eX) + i * n;
    const int q0 = 8 * (sec ? k - nb : k);
    uint32_t v = 0;
    for (int j = 0; j < 8 && q0 + j < n; ++j) v |= (uint32_t)(e[q0 + j] & 1) << j;
    out[k] = (uint8_t)v;
}

}  // namespace

// ---- host side ----------------------------------------------------------------------------------
// Why this code cannot take the kernel at QEC_OPT_OSD_ORDER = order (empty: it can).
std::string osd_dev_unsupported(const OsdPlan& P, int order, bool weighted)
{
    const int n = P.sec[0].n, mmax = std::max(P.sec[0].m, P.sec[1].m);
    if (n > kOsdMaxN || mmax > kOsdMaxN)
        return "OSD: n = " + std::to_string(n) + ", " + std::to_string(mmax) + " checks; the kernel takes up to " +
               std::to_string(kOsdMaxN) + " of each";
    if (order > 0 && n < 2) return "OSD: the combination sweep takes codes of n >= 2";
    const int W = P.sec[0].W;
    const size_t bytes = 4 * (size_t)osd_lds_words(mmax, n, W | 1, order, weighted);
    if (bytes > kOsdMaxLds) {
        if (order > 0 && weighted && 4 * (size_t)osd_lds_words(mmax, n, W | 1, order) <= kOsdMaxLds)
            return "OSD: the sweep fits in LDS at QEC_OPT_OSD_ORDER = " + std::to_string(order) +
                   " under the Hamming score, but not with the weighted score's arrays (QEC_OPT_OSD_SCORE = 1 with priors): " +
                   std::to_string(bytes) + " B, one workgroup has " + std::to_string(kOsdMaxLds);
        return "OSD: the augmented matrix" + std::string(order > 0 ? " and the sweep's column vectors need " : " needs ") +
               std::to_string(bytes) + " B of LDS, one workgroup has " + std::to_string(kOsdMaxLds);
    }
    return std::string();
}

// Uploads the plan's tables to the current device.  nullptr (error text set) on failure.
OsdDevPlan* osd_dev_create(const OsdPlan& P)
{
    auto* D = new OsdDevPlan;
    const int n = P.sec[0].n, W = P.sec[0].W;
    size_t off[5] = {0};
    for (int s = 0; s < 2; ++s) {
        off[2 * s + 1] = off[2 * s] + ((P.sec[s].H.size() * 4 + 255) / 256) * 256;
        off[2 * s + 2] = off[2 * s + 1] + (((size_t)n * 4 + 255) / 256) * 256;
    }
    if (hipMalloc(&D->mem, std::max<size_t>(off[4], 256)) != hipSuccess) {
        delete D;
        fail(QEC_ERR_NOMEM, "OSD tables: hipMalloc");
        return nullptr;
    }
    char* base = static_cast<char*>(D->mem);
    for (int s = 0; s < 2; ++s) {
        const OsdSector& S = P.sec[s];
        if ((S.H.size() && hipMemcpy(base + off[2 * s], S.H.data(), S.H.size() * 4, hipMemcpyHostToDevice) != hipSuccess) ||
            (n && hipMemcpy(base + off[2 * s + 1], S.qpos.data(), (size_t)n * 4, hipMemcpyHostToDevice) != hipSuccess)) {
            (void)hipFree(D->mem);
            delete D;
            fail(QEC_ERR_HIP, "OSD tables: upload");
            return nullptr;
        }
        D->d.H[s] = reinterpret_cast<const uint32_t*>(base + off[2 * s]);
        D->d.qpos[s] = reinterpret_cast<const int32_t*>(base + off[2 * s + 1]);
        D->d.m[s] = S.m;
        D->d.rank[s] = S.rank;
    }
    D->d.n = n;
    D->d.W = W;
    D->d.Ws = W | 1;
    D->d.qn = (long long)P.qn;
    D->mmax = std::max(P.sec[0].m, P.sec[1].m);
    D->lds_bytes = 4 * osd_lds_words(D->mmax, n, D->d.Ws, 0);
    return D;
}

void osd_dev_free(OsdDevPlan* D)
{
    if (!D) return;
    (void)hipFree(D->mem);
    delete D;
}

int launch_osd(const OsdDevPlan* D, int sweep, int order, const uint8_t* sX, const uint8_t* sZ, long long B,
               const float* q, uint8_t* eX, uint8_t* eZ, uint8_t* flags, uint32_t* repaired, uint32_t* swept,
               const int32_t* w, hipStream_t st, bool llr)
{
    if (B <= 0) return QEC_OK;
    if (B >= (1LL << 30)) return fail(QEC_ERR_ARG, "OSD: batch too large");
    OsdDev P = D->d;
    P.sweep = sweep;
    if (order <= 0) {
        if (llr)
            hipLaunchKernelGGL((osd_kernel<false, false, true>), dim3((unsigned)(2 * B)), dim3(64), D->lds_bytes, st, P, sX,
                               sZ, B, q, eX, eZ, flags, repaired, OsdCs{}, nullptr, nullptr);
        else
            hipLaunchKernelGGL(osd_kernel<false>, dim3((unsigned)(2 * B)), dim3(64), D->lds_bytes, st, P, sX, sZ, B, q, eX,
                               eZ, flags, repaired, OsdCs{}, nullptr, nullptr);
        return launch_check("osd0");
    }
    // the sweep's column vectors behind the elimination's image (QEC_OPT_OSD_ORDER is refused where
    // the sum does not fit: osd_dev_unsupported)
    const uint32_t lds = 4 * osd_lds_words(D->mmax, P.n, P.Ws, order, w != nullptr);
    if (order > kOsdMaxOrder || lds > kOsdMaxLds)
        return fail(QEC_ERR_UNSUPPORTED, w ? "OSD: the sweep with the weighted score's arrays does not fit in LDS"
                                           : "OSD: the sweep does not fit in LDS");
    const OsdCs C{order, osd_rws(D->mmax)};
    if (w) {  // QEC_OPT_OSD_SCORE = 1 with priors set: the weight tables [2][n]
        if (llr)
            hipLaunchKernelGGL((osd_kernel<true, true, true>), dim3((unsigned)(2 * B)), dim3(64), lds, st, P, sX, sZ, B, q,
                               eX, eZ, flags, repaired, C, swept, w);
        else
            hipLaunchKernelGGL((osd_kernel<true, true>), dim3((unsigned)(2 * B)), dim3(64), lds, st, P, sX, sZ, B, q, eX, eZ,
                               flags, repaired, C, swept, w);
        return launch_check("osd_cs_weighted");
    }
    if (llr)
        hipLaunchKernelGGL((osd_kernel<true, false, true>), dim3((unsigned)(2 * B)), dim3(64), lds, st, P, sX, sZ, B, q, eX,
                           eZ, flags, repaired, C, swept, nullptr);
    else
        hipLaunchKernelGGL(osd_kernel<true>, dim3((unsigned)(2 * B)), dim3(64), lds, st, P, sX, sZ, B, q, eX, eZ, flags,
                           repaired, C, swept, nullptr);
    return launch_check("osd_cs");
}

int launch_osd_collect(const uint8_t* rec, int rstride, int n, long long B, int32_t* list, uint32_t* count,
                       hipStream_t st)
{
    if (B <= 0) return QEC_OK;
    hipLaunchKernelGGL(osd_collect_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, rec, rstride,
                       2 * ((n + 7) / 8), B, list, count);
    return launch_check("osd_collect");
}

int launch_osd_gather(const int32_t* list, long long cnt, const uint8_t* sX, const uint8_t* sZ, bool bits, int mX,
                      int mZ, const uint8_t* rec, int rstride, int n, uint8_t* oX, uint8_t* oZ, uint8_t* fl,
                      uint8_t* fl0, hipStream_t st)
{
    if (cnt <= 0) return QEC_OK;
    hipLaunchKernelGGL(osd_gather_kernel, dim3((unsigned)cnt), dim3(128), 0, st, list, cnt, sX, sZ, bits ? 1 : 0, mX,
                       mZ, rec, rstride, 2 * ((n + 7) / 8), oX, oZ, fl, fl0);
    return launch_check("osd_gather");
}

int launch_osd_scatter(const int32_t* list, long long cnt, const uint8_t* eX, const uint8_t* eZ, const uint8_t* fl,
                       const uint8_t* fl0, int n, uint8_t* rec, int rstride, hipStream_t st)
{
    if (cnt <= 0) return QEC_OK;
    const long long total = cnt * (2 * ((n + 7) / 8) + 1);
    hipLaunchKernelGGL(osd_scatter_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, list, cnt, eX, eZ,
                       fl, fl0, n, rec, rstride);
    return launch_check("osd_scatter");
}

}  // namespace qec
