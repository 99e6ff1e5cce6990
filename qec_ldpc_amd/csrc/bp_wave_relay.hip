// Register-resident Relay-BP for circulant-permutation codes (QEC_OPT_RELAY_WAVE; DESIGN.md section 2, "The relay form
// in the wave layout").  The rule is sp_relay_decode's (bp_sparse.hip) in every bit; the layout is bp_wave_minsum.hip's,
// whose lane helpers are restated here (wr_*) so that file, and its kernels' instruction streams, stay as they are:
//   * one 64-lane wave owns G = 64 / P syndrome pairs, lane g P + i is circulant row i of pair g; sector X is decoded
//     first, then sector Z.  Check view: the R L slots of the lane's checks in VGPRs.  Variable view: per column l the
//     channel LLR, the relay's memory M and one decision bit, all in VGPRs; gathers by ds_bpermute_b32.
//   * per group (the same on all its lanes): act, the leg, the iteration within the leg, the iteration total, the
//     solution count and the best weight.  Groups of one wave may be in different legs, so the gamma of a variable
//     pass is loaded behind a per-lane address, by live lanes only; it is re-read every pass (L2 / L1 hits) instead of
//     being held in L more registers.
//   * there is no workspace: M and the best solution's decisions (one word) are registers.
// No LDS beyond the permutes' crossbar, no atomics, no barriers, no scratch.  The loop of a sector leaves when a ballot
// of act is empty and carries the trip bound legs x max(maxIter, 1); every inner loop is bounded by template constants.
//
// Groups of one wave finish at different times under every stop rule (different numbers of legs): control flow stays
// wave-uniform, every lane executes every pass and every permute with EXEC full, and a finished group's registers
// (slots, M, decisions, best, counters) are kept by selects.  With G = 1 nothing is ever frozen, the group's predicates
// are wave-uniform (taken over group 0's lanes by a scalar mask) and the selects are not compiled in.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>

#include "qec_internal.h"

#pragma clang fp contract(off)

namespace qec {

constexpr int kWrMaxR = 6, kWrMaxL = 12, kWrMaxRL = 72;  // the largest shape of the table below, (4,6,12)

struct WaveRelayArgs {
    const uint8_t* sX;
    const uint8_t* sZ;
    uint8_t* eX;
    uint8_t* eZ;
    uint8_t* flags;
    int32_t* iters;          // nullable
    float* q;                // nullable
    const float* llr;        // null: the scalar lam; else the channel LLRs, sector X [n] then Z [n]
    const float* gamma;      // [legs][sector][n]
    const int32_t* weight;   // null (w_v = 1), or sector X [n] then Z [n]: the handle's integer weight tables
    long long B;
    int P, G, n, mX, mZ;
    float lam, alpha;
    int maxIter, legs, solutions;
    // lane-relabelled circulant tables (wr_relabel below)
    int SX[kWrMaxRL], SZ[kWrMaxRL];  // rotation of block (r, l) between check and variable views
    int DX[kWrMaxR], DZ[kWrMaxR];    // check-view lane lambda holds check (r, (lambda + D[r]) mod P)
    int CX[kWrMaxL], CZ[kWrMaxL];    // var-view lane mu holds variable (l, (mu + C[l]) mod P)
};

// wm_relabel of bp_wave_minsum.hip: S[r][l] = (E[r][l] + D[r] - C[l]) mod P with C[l] = E[0][l] and
// D[r] = (C[0] - E[r][0]) mod P, so the blocks of row 0 and column 0 need no rotation
static void wr_relabel(const int* E, int R, int L, int P, int* S, int* D, int* C)
{
    for (int l = 0; l < L; ++l) C[l] = E[l];
    for (int r = 0; r < R; ++r) D[r] = ((C[0] - E[r * L]) % P + P) % P;
    for (int r = 0; r < R; ++r)
        for (int l = 0; l < L; ++l) S[r * L + l] = ((E[r * L + l] + D[r] - C[l]) % P + P) % P;
}

struct WrLane {
    int i;       // in-group index (an idle lane: its index above the last group)
    int b0, b1;  // bpermute bases 4 (gb + i) and 4 (gb + i + P)
    unsigned long long gm;   // the lanes of this lane's group
    unsigned long long gm0;  // the lanes of group 0 (wave-uniform)
    bool live;   // the lane belongs to a syndrome pair of the batch
};

// The value of lane gb + (i - s) mod P of this lane's group, s in [0, P] (0 and P: the lane's own)
__device__ __forceinline__ int wr_rot_i(int v, const WrLane& ln, int s)
{
    const int base = ln.i < s ? ln.b1 : ln.b0;
    return __builtin_amdgcn_ds_bpermute(base + (256 - 4 * s), v);
}
__device__ __forceinline__ float wr_rot(float v, const WrLane& ln, int s)
{
    return __int_as_float(wr_rot_i(__float_as_int(v), ln, s));
}
__device__ __forceinline__ int wr_wrap(int x, int P) { return x >= P ? x - P : x; }
// Whether pred holds on every lane of the lane's group; with one group per wave (FREEZE off) of group 0, wave-uniform
template <bool FREEZE>
__device__ __forceinline__ bool wr_group_all(bool pred, const WrLane& ln)
{
    return (__builtin_amdgcn_ballot_w64(!pred) & (FREEZE ? ln.gm : ln.gm0)) == 0ull;
}
__device__ __forceinline__ bool wr_inside(float x) { return __builtin_fabsf(x) < kMinSumInside; }

// The sector's shift table, read from the kernel-argument segment behind an offset laundered once per use (wm_table)
typedef const int __attribute__((address_space(4))) wr_kernarg_int;
struct WrTable {
    wr_kernarg_int* t;
    __device__ __forceinline__ int operator[](int k) const { return t[k]; }
};
template <int SEC>
__device__ __forceinline__ WrTable wr_table()
{
    int off = (int)((SEC ? offsetof(WaveRelayArgs, SZ) : offsetof(WaveRelayArgs, SX)) / sizeof(int));
    asm volatile("" : "+s"(off));
    return WrTable{(wr_kernarg_int*)__builtin_amdgcn_kernarg_segment_ptr() + off};
}

// sp_minsum_check for the lane's R checks; sb holds their syndrome entries (two bits each: 0, 1, 2 = any other value)
template <int R, int L, bool FREEZE>
__device__ __forceinline__ void wr_check_pass(float (&m)[R][L], uint32_t sb, float alpha, bool act)
{
#pragma unroll
    for (int r = 0; r < R; ++r) {
        uint32_t min1 = kMinSumCap, min2 = kMinSumCap;
        uint32_t sgn = ((sb >> (2 * r)) & 3u) != 0u ? 0x80000000u : 0u;  // the parity, kept in the sign position
        int arg = -1;
#pragma unroll
        for (int l = 0; l < L; ++l) {
            const uint32_t b = __float_as_uint(m[r][l]);
            const uint32_t x = b & 0x7FFFFFFFu;
            sgn ^= b;
            const bool lt1 = x < min1;
            min2 = lt1 ? min1 : (x < min2 ? x : min2);
            arg = lt1 ? l : arg;
            min1 = lt1 ? x : min1;
        }
        sgn &= 0x80000000u;
        const uint32_t o1 = __float_as_uint(alpha * __uint_as_float(min1));
        const uint32_t o2 = __float_as_uint(alpha * __uint_as_float(min2));
#pragma unroll
        for (int l = 0; l < L; ++l) {
            const uint32_t b = __float_as_uint(m[r][l]);
            const uint32_t o = (l == arg ? o2 : o1) | ((sgn ^ b) & 0x80000000u);
            m[r][l] = __uint_as_float(FREEZE && !act ? b : o);
        }
    }
}

// sp_relay_var for the lane's L variables in leg `leg`: the gamma loads, the bias, the gathers, the folds from the
// bias, M = the posterior, the inverse rotations.  `last` (per lane: the group's iteration N - 1 of its leg) gives every
// slot the posterior -- the fold that ends the extrinsic pass -- by select.  Returns the decisions (bit l).
template <int R, int L, int SEC, bool FREEZE>
__device__ __forceinline__ uint32_t wr_var_pass(const WaveRelayArgs& a, float (&m)[R][L], const float (&lamv)[L],
                                                float (&mem)[L], const WrLane& ln, bool act, bool last, int leg,
                                                uint32_t hd_old)
{
    const int P = a.P;
    const int* C = SEC ? a.CZ : a.CX;
    const WrTable S = wr_table<SEC>();
    float gam[L];
#pragma unroll
    for (int l = 0; l < L; ++l) gam[l] = 0.0f;
    if (ln.live) {  // the permutes below run with EXEC full again
        const float* t = a.gamma + ((size_t)leg * 2 + SEC) * (size_t)a.n;
#pragma unroll
        for (int l = 0; l < L; ++l) gam[l] = t[l * P + wr_wrap(ln.i + C[l], P)];
    }
    uint32_t hd = 0;
#pragma unroll
    for (int l = 0; l < L; ++l) {
        float g[R], o[R];
#pragma unroll
        for (int r = 0; r < R; ++r) g[r] = (r == 0 || l == 0) ? m[r][l] : wr_rot(m[r][l], ln, S[r * L + l]);
        const float t0 = 1.0f - gam[l];
        const float t1 = t0 * lamv[l];
        const float t2 = gam[l] * mem[l];
        float post = t1 + t2;
        post = post + 0.0f;  // -0.0f becomes +0.0f
#pragma unroll
        for (int j = 0; j < R; ++j) {
            float t = post;  // b + g_0 + ... + g_{j-1}
#pragma unroll
            for (int k = j + 1; k < R; ++k) t = t + g[k];
            o[j] = t;
            post = post + g[j];
        }
        hd |= (uint32_t)(post < 0.0f) << l;
        mem[l] = FREEZE && !act ? mem[l] : post;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float out = last ? post : o[r];
            const float back = (r == 0 || l == 0) ? out : wr_rot(out, ln, P - S[r * L + l]);
            m[r][l] = FREEZE && !act ? m[r][l] : back;
        }
    }
    return FREEZE && !act ? hd_old : hd;
}

// Whether the parities of the lane's R checks over the decisions hd (variable view, bit l) equal their syndrome
// entries; an entry other than 0 / 1 equals no parity
template <int R, int L, int SEC>
__device__ __forceinline__ bool wr_lane_syndrome_ok(const WaveRelayArgs& a, uint32_t hd, uint32_t sb, const WrLane& ln)
{
    const int P = a.P;
    const WrTable S = wr_table<SEC>();
    bool ok = true;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        uint32_t x = 0;
#pragma unroll
        for (int l = 0; l < L; ++l) {
            const uint32_t h = (r == 0 || l == 0) ? hd : (uint32_t)wr_rot_i((int)hd, ln, P - S[r * L + l]);
            x ^= (h >> l) & 1u;
        }
        ok &= x == ((sb >> (2 * r)) & 3u);
    }
    return ok;
}

template <int R, int L>
__device__ __forceinline__ bool wr_lane_any_inside(const float (&m)[R][L])
{
    bool in = false;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int l = 0; l < L; ++l) in |= wr_inside(m[r][l]);
    return in;
}

// The sum over the lanes of the lane's group of x, modulo 2^32, from BITS ballots: bit j of the sum's terms is set on
// popcount(ballot & group) lanes.  Integer adds, so the order does not matter; x < 2^BITS on every lane.
template <int BITS, bool FREEZE>
__device__ __forceinline__ uint32_t wr_group_sum(uint32_t x, const WrLane& ln)
{
    const unsigned long long gm = FREEZE ? ln.gm : ln.gm0;
    uint32_t s = 0;
#pragma unroll
    for (int j = 0; j < BITS; ++j) {
        const unsigned long long bal = __builtin_amdgcn_ballot_w64(((x >> j) & 1u) != 0u) & gm;
        s += (uint32_t)__builtin_popcountll(bal) << j;
    }
    return s;
}

// The slots at the start of a leg, for the lanes with `sel`: every slot at its variable's channel LLR (under a table
// the (R - 1)(L - 1) rotations of the LLRs into the check view, executed by the whole wave)
template <int R, int L, int SEC>
__device__ __forceinline__ void wr_init_slots(const WaveRelayArgs& a, float (&m)[R][L], const float (&lamv)[L],
                                              const WrLane& ln, bool sel)
{
    const int P = a.P;
    const WrTable S = wr_table<SEC>();
    if (a.llr != nullptr) {  // wave-uniform
#pragma unroll
        for (int l = 0; l < L; ++l)
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float x = (r == 0 || l == 0) ? lamv[l] : wr_rot(lamv[l], ln, P - S[r * L + l]);
                m[r][l] = sel ? x : m[r][l];
            }
    } else {
#pragma unroll
        for (int l = 0; l < L; ++l)
#pragma unroll
            for (int r = 0; r < R; ++r) m[r][l] = sel ? lamv[l] : m[r][l];
    }
}

// One sector of the wave's syndrome pairs, start to outputs; returns the sector's flag bits and, through itn, its
// iteration count over all legs (both per lane, the same on every lane of a group)
template <int R, int L, int SEC, int STOP, bool FREEZE>
__device__ __forceinline__ uint32_t wr_sector(const WaveRelayArgs& a, const WrLane& ln, long long b, int& itn)
{
    const int P = a.P, n = a.n, N = a.maxIter;
    const int legs = a.legs, sols_max = a.solutions;
    const int m_s = SEC ? a.mZ : a.mX;
    const int* D = SEC ? a.DZ : a.DX;
    const int* C = SEC ? a.CZ : a.CX;
    const float alpha = a.alpha;
    const bool weigh = sols_max > 1;  // wave-uniform

    // syndrome entries of the lane's checks (r, (i + D[r]) mod P)
    uint32_t sb = 0;
    if (ln.live) {
        const uint8_t* s = (SEC ? a.sZ : a.sX) + b * m_s;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint32_t v = s[r * P + wr_wrap(ln.i + D[r], P)];
            sb |= (v > 1u ? 2u : v) << (2 * r);
        }
    }
    // channel LLRs of the lane's variables (l, (i + C[l]) mod P); leg 0: M = lambda, the decisions of N = 0
    float lamv[L], mem[L];
#pragma unroll
    for (int l = 0; l < L; ++l) lamv[l] = a.lam;
    if (a.llr != nullptr && ln.live) {
        const float* t = a.llr + (size_t)SEC * n;
#pragma unroll
        for (int l = 0; l < L; ++l) lamv[l] = t[l * P + wr_wrap(ln.i + C[l], P)];
    }
    uint32_t hd = 0, best = 0;
#pragma unroll
    for (int l = 0; l < L; ++l) {
        mem[l] = lamv[l];
        hd |= (uint32_t)(lamv[l] < 0.0f) << l;
    }
    float m[R][L];
    wr_init_slots<R, L, SEC>(a, m, lamv, ln, true);

    // per group: the same on every lane of a group (with FREEZE off: wave-uniform)
    bool act = FREEZE ? ln.live : true;
    int leg = 0, k = 0, sols = 0;
    uint32_t wbest = 0u;
    itn = 0;
    const long long bound = (long long)legs * (N > 1 ? N : 1);
    for (long long trip = 0; trip < bound; ++trip) {
        if (__builtin_amdgcn_ballot_w64(act) == 0ull) break;
        bool bad = true;  // SYNDROME: of this trip's decisions
        if (N > 0) {
            const bool last = k == N - 1;
            itn += act ? 1 : 0;
            wr_check_pass<R, L, FREEZE>(m, sb, alpha, act);
            hd = wr_var_pass<R, L, SEC, FREEZE>(a, m, lamv, mem, ln, act, last, leg, hd);
            k += act ? 1 : 0;
        }
        // which groups end their leg here (the call's stop rule, counted within the leg)
        bool end = act && k == N;
        if (STOP == QEC_STOP_REF && N > 0) {
            const bool t = act && (k - 1) % 10 == 0;
            if (__builtin_amdgcn_ballot_w64(t) != 0ull) {
                const bool out = wr_group_all<FREEZE>(!wr_lane_any_inside<R, L>(m), ln);
                if (t && out) end = true;
            }
        } else if (STOP == QEC_STOP_SYNDROME && N > 0) {
            bad = !wr_group_all<FREEZE>(wr_lane_syndrome_ok<R, L, SEC>(a, hd, sb, ln), ln);
            if (act && !bad) end = true;
        }
        if (__builtin_amdgcn_ballot_w64(end) == 0ull) continue;

        // ---- the end of a leg: a solution?  the next leg, or the end of the group's relay ----
        if (STOP != QEC_STOP_SYNDROME || N == 0)
            bad = !wr_group_all<FREEZE>(wr_lane_syndrome_ok<R, L, SEC>(a, hd, sb, ln), ln);
        const bool solved = end && !bad;
        uint32_t W = 0u;
        if (weigh && __builtin_amdgcn_ballot_w64(solved) != 0ull) {
            if (a.weight != nullptr) {
                uint32_t x = 0u;
                if (ln.live) {
                    const int32_t* w = a.weight + (size_t)SEC * n;
#pragma unroll
                    for (int l = 0; l < L; ++l)
                        x += ((hd >> l) & 1u) ? (uint32_t)w[l * P + wr_wrap(ln.i + C[l], P)] : 0u;
                }
                W = wr_group_sum<32, FREEZE>(x, ln);
            } else {
                W = wr_group_sum<4, FREEZE>((uint32_t)__builtin_popcount(hd), ln);  // at most L <= 12 < 16 per lane
            }
        }
        const bool keep = solved && (sols == 0 || W < wbest);  // ties keep the earlier leg
        wbest = keep ? W : wbest;
        best = keep ? hd : best;
        sols += solved ? 1 : 0;
        const bool done = end && (sols == sols_max || leg == legs - 1 || N == 0);
        const bool next = end && !done;
        act = done ? false : act;
        leg += next ? 1 : 0;
        k = next ? 0 : k;
        if (__builtin_amdgcn_ballot_w64(next) != 0ull) wr_init_slots<R, L, SEC>(a, m, lamv, ln, next);
    }

    // ---- the final state: the last executed leg's slots and decisions, the best solution ----
    const bool convFail = !wr_group_all<FREEZE>(!wr_lane_any_inside<R, L>(m), ln);
    if (ln.live) {
        const uint32_t h = sols ? best : hd;
        uint8_t* e = (SEC ? a.eZ : a.eX) + b * n;
#pragma unroll
        for (int l = 0; l < L; ++l) e[l * P + wr_wrap(ln.i + C[l], P)] = (uint8_t)((h >> l) & 1u);
        if (a.q != nullptr) {
            float* q = a.q + b * ((long long)(a.mX + a.mZ) * L) + (SEC ? (long long)a.mX * L : 0);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float* row = q + (size_t)(r * P + wr_wrap(ln.i + D[r], P)) * L;
#pragma unroll
                for (int l = 0; l < L; ++l) row[l] = m[r][l];
            }
        }
    }
    uint32_t f = 0;
    if (sols == 0) f |= SEC ? QEC_SYNDROME_FAIL_Z : QEC_SYNDROME_FAIL_X;
    if (convFail) f |= SEC ? QEC_CONVERGENCE_FAIL_Z : QEC_CONVERGENCE_FAIL_X;
    return f;
}

template <int J, int K, int L, int STOP>
__global__ __launch_bounds__(64) void wave_relay_kernel(const WaveRelayArgs a)
{
    const int lane = (int)threadIdx.x, P = a.P, G = a.G;
    const int g = lane / P;  // G for an idle lane
    WrLane ln;
    ln.i = lane - g * P;
    ln.b0 = 4 * lane;
    ln.b1 = ln.b0 + 4 * P;
    ln.gm0 = P >= 64 ? ~0ull : ((1ull << P) - 1ull);
    ln.gm = ln.gm0 << (g * P);
    const long long b = (long long)blockIdx.x * G + g;
    ln.live = g < G && b < a.B;

    uint32_t f;
    int itX, itZ;
    if (G > 1) {  // wave-uniform: groups that finish on their own, under every stop rule
        f = wr_sector<J, L, 0, STOP, true>(a, ln, b, itX);
        f |= wr_sector<K, L, 1, STOP, true>(a, ln, b, itZ);
    } else {
        f = wr_sector<J, L, 0, STOP, false>(a, ln, b, itX);
        f |= wr_sector<K, L, 1, STOP, false>(a, ln, b, itZ);
    }
    if (ln.live && ln.i == 0) {
        a.flags[b] = (uint8_t)f;
        if (a.iters != nullptr) { a.iters[2 * b] = itX; a.iters[2 * b + 1] = itZ; }
    }
}

// ---- host side ---------------------------------------------------------------
struct WaveRelayShape {
    int J, K, L;
    const void* fn[3];  // by stop rule
};

template <int J, int K, int L>
static WaveRelayShape wr_shape()
{
    WaveRelayShape s{J, K, L, {nullptr, nullptr, nullptr}};
    s.fn[QEC_STOP_REF] = reinterpret_cast<const void*>(&wave_relay_kernel<J, K, L, QEC_STOP_REF>);
    s.fn[QEC_STOP_FIXED] = reinterpret_cast<const void*>(&wave_relay_kernel<J, K, L, QEC_STOP_FIXED>);
    s.fn[QEC_STOP_SYNDROME] = reinterpret_cast<const void*>(&wave_relay_kernel<J, K, L, QEC_STOP_SYNDROME>);
    return s;
}

// the block shapes of kWaveMinsumShapes (bp_wave_minsum.hip)
static const WaveRelayShape kWaveRelayShapes[] = {
    wr_shape<4, 5, 10>(), wr_shape<3, 3, 6>(), wr_shape<2, 3, 6>(), wr_shape<3, 4, 8>(),
    wr_shape<4, 4, 8>(),  wr_shape<3, 5, 10>(), wr_shape<4, 6, 12>(), wr_shape<2, 2, 4>(),
};

// The wave relay kernels of a code, or nullptr: the codes of select_wave_minsum.  No HIP call.
const void* select_wave_relay(const Code& c)
{
    if (c.general || !c.is_qc || c.P > 64 || c.P < 1) return nullptr;
    if (c.J > kWrMaxR || c.K > kWrMaxR || c.L > kWrMaxL || c.J * c.L > kWrMaxRL || c.K * c.L > kWrMaxRL) return nullptr;
    if ((int)c.EX.size() != c.J * c.L || (int)c.EZ.size() != c.K * c.L) return nullptr;
    for (const WaveRelayShape& s : kWaveRelayShapes)
        if (s.J == c.J && s.K == c.K && s.L == c.L) return &s;
    return nullptr;
}

// "wave-relay J=.. K=.. L=.. P=.. G=.." for qec_decoder_describe
std::string wave_relay_name(const Code& c)
{
    char buf[96];
    snprintf(buf, sizeof buf, "wave-relay J=%d K=%d L=%d P=%d G=%d", c.J, c.K, c.L, c.P, 64 / c.P);
    return buf;
}

// One relay decode launch in the wave layout: d as launch_decode_sparse's RELAY kernels read it (minsum = the scale,
// lam, with prior set llr, gamma = the tables, legs, solutions, relay_weight).  It allocates nothing.  One wave per
// workgroup, ceil(B / G) workgroups.
int launch_wave_relay(const void* shape, const Code& c, const SparseDecode& d, hipStream_t stream)
{
    const WaveRelayShape* s = static_cast<const WaveRelayShape*>(shape);
    if (d.B <= 0) return QEC_OK;
    if (s == nullptr || s->J != c.J || s->K != c.K || s->L != c.L || c.P < 1 || c.P > 64)
        return fail(QEC_ERR_ARG, "wave relay launch: the kernels are another code's");
    if (!d.minsum || d.gamma == nullptr || d.corr || d.serial)
        return fail(QEC_ERR_ARG, "wave relay launch: min-sum with relay tables only (no correlated form or serial schedule)");
    if (d.legs < 1 || d.legs > kRelayMaxLegs || d.solutions < 1 || d.solutions > kRelayMaxSolutions)
        return fail(QEC_ERR_ARG, "wave relay launch: the relay needs its tables (qec_decoder_set_relay)");
    if (d.stop < 0 || d.stop > 2) return fail(QEC_ERR_ARG, "wave relay launch: unknown stop rule");
    if (d.prior != nullptr && d.llr == nullptr)
        return fail(QEC_ERR_ARG, "wave relay launch: min-sum under priors needs its LLR tables");
    WaveRelayArgs a{};
    a.sX = d.sX; a.sZ = d.sZ; a.eX = d.eX; a.eZ = d.eZ; a.flags = d.flags; a.iters = d.iters; a.q = d.q;
    a.llr = d.prior != nullptr ? d.llr : nullptr;
    a.gamma = d.gamma;
    a.weight = d.relay_weight;
    a.B = d.B;
    a.P = c.P; a.G = 64 / c.P; a.n = c.n; a.mX = c.mX; a.mZ = c.mZ;
    a.lam = d.lam;
    a.alpha = (float)d.minsum / 256.0f;
    a.maxIter = d.maxIter < 0 ? 0 : d.maxIter;
    a.legs = d.legs;
    a.solutions = d.solutions;
    wr_relabel(c.EX.data(), c.J, c.L, c.P, a.SX, a.DX, a.CX);
    wr_relabel(c.EZ.data(), c.K, c.L, c.P, a.SZ, a.DZ, a.CZ);
    const long long waves = (d.B + a.G - 1) / a.G;
    if (waves > 0x7fffffffLL) return fail(QEC_ERR_ARG, "wave relay launch: batch too large for one launch");
    void* args[] = {&a};
    (void)hipLaunchKernel(s->fn[d.stop], dim3((unsigned)waves), dim3(64), args, 0, stream);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(QEC_ERR_HIP, std::string("wave relay launch: ") + hipGetErrorString(err));
    return QEC_OK;
}

}  // namespace qec
