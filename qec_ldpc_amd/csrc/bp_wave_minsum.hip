// Register-resident scaled min-sum for circulant-permutation codes (QEC_OPT_MINSUM_WAVE; DESIGN.md section 2,
// "The min-sum form in the wave layout").  The rule is sp_minsum_decode's (bp_sparse.hip) in every bit; the layout is
// bp_decode.hip's:
//   * one 64-lane wave owns G = 64 / P syndrome pairs, lane g P + i is circulant row i of pair g; the 64 - G P lanes
//     above the groups are idle (they compute on zeros and write nothing).  Sector X is decoded first, then sector Z.
//   * check view: lane i holds, in VGPRs, the message of every edge (r, l, i) of the sector -- check (r, i) <-> variable
//     (l, (E[r][l] + i) mod P) -- for all iterations.  A check's slots in ascending variable order are the column
//     blocks l = 0 .. L-1, so sp_minsum_check's one pass over the row (first minimum, second minimum, argmin on bit
//     patterns, the parity seeded with the syndrome bit, two multiplies by alpha) runs over L registers of the lane.
//   * variable view: lane j holds variable (l, j) of every column l: its channel LLR (L registers, loaded once per
//     sector from the scalar or from the handle's table) and, during a column's update, its R incoming messages,
//     gathered by the block rotations (ds_bpermute_b32).  A variable's messages in ascending check order are the row
//     blocks r = 0 .. R-1, so sp_minsum_var's left folds from lambda run as they stand; the outputs go back with the
//     inverse rotations.
//   * relabel() (restated from bp_decode.hip) makes the blocks of row 0 and column 0 rotation-free.
// No LDS beyond the permutes' crossbar, no atomics, no barriers, no scratch.  Every loop is bounded by maxIter.
//
// Groups of one wave stop on their own (G > 1, reference and syndrome stop): control flow stays wave-uniform, every
// lane executes every pass, and a finished group's registers (messages, decisions, count) are kept by selects, so a
// permute never runs with part of a group's lanes disabled.  The wave leaves the loop when no live group runs.  With
// G = 1 or under the fixed stop nothing is ever frozen and the selects are not compiled in (a wave-uniform branch
// on G picks the body).
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>

#include "qec_internal.h"

#pragma clang fp contract(off)

namespace qec {

constexpr int kWmMaxR = 6, kWmMaxL = 12, kWmMaxRL = 72;  // the largest shape of the table below, (4,6,12)

struct WaveMinsumArgs {
    const uint8_t* sX;
    const uint8_t* sZ;
    uint8_t* eX;
    uint8_t* eZ;
    uint8_t* flags;
    int32_t* iters;      // nullable
    float* q;            // nullable
    const float* llr;    // null: the scalar lam; else the channel LLRs, sector X [n] then Z [n]
    long long B;
    int P, G, n, mX, mZ;
    float lam, alpha;
    int maxIter;
    // lane-relabelled circulant tables (relabel below)
    int SX[kWmMaxRL], SZ[kWmMaxRL];  // rotation of block (r, l) between check and variable views
    int DX[kWmMaxR], DZ[kWmMaxR];    // check-view lane lambda holds check (r, (lambda + D[r]) mod P)
    int CX[kWmMaxL], CZ[kWmMaxL];    // var-view lane mu holds variable (l, (mu + C[l]) mod P)
};

// Block (r, l) of a sector is the circulant "check (r, i) <-> variable (l, (E[r][l] + i) mod P)".  Storing check
// (r, i) in lane (i - D[r]) mod P and variable (l, j) in lane (j - C[l]) mod P turns the block's check->variable lane
// rotation into S[r][l] = (E[r][l] + D[r] - C[l]) mod P.  With C[l] = E[0][l] and D[r] = (C[0] - E[r][0]) mod P the
// R + L - 1 blocks of row 0 and column 0 need no rotation.  Arithmetic (and so every output bit) is unchanged.
static void wm_relabel(const int* E, int R, int L, int P, int* S, int* D, int* C)
{
    for (int l = 0; l < L; ++l) C[l] = E[l];
    for (int r = 0; r < R; ++r) D[r] = ((C[0] - E[r * L]) % P + P) % P;
    for (int r = 0; r < R; ++r)
        for (int l = 0; l < L; ++l) S[r * L + l] = ((E[r * L + l] + D[r] - C[l]) % P + P) % P;
}

struct WmLane {
    int i;       // in-group index (an idle lane: its index above the last group)
    int b0, b1;  // bpermute bases 4 (gb + i) and 4 (gb + i + P)
    unsigned long long gm;  // the lanes of this lane's group
    bool live;   // the lane belongs to a syndrome pair of the batch
};

// The value of lane gb + (i - s) mod P of this lane's group, s in [0, P] (0 and P: the lane's own).  ds_bpermute
// selects lane (addr >> 2) & 63; the +256 keeps the address non-negative.
__device__ __forceinline__ int wm_rot_i(int v, const WmLane& ln, int s)
{
    const int base = ln.i < s ? ln.b1 : ln.b0;
    return __builtin_amdgcn_ds_bpermute(base + (256 - 4 * s), v);
}
__device__ __forceinline__ float wm_rot(float v, const WmLane& ln, int s)
{
    return __int_as_float(wm_rot_i(__float_as_int(v), ln, s));
}
__device__ __forceinline__ int wm_wrap(int x, int P) { return x >= P ? x - P : x; }
__device__ __forceinline__ bool wm_group_all(bool pred, const WmLane& ln)
{
    return (__builtin_amdgcn_ballot_w64(!pred) & ln.gm) == 0ull;
}
__device__ __forceinline__ bool wm_inside(float x) { return __builtin_fabsf(x) < kMinSumInside; }

// The sector's shift table, read from the kernel-argument segment (the kernel's one argument starts at its offset 0)
// behind an offset laundered once per use (it is 0), so that the R L shift loads and rotation addresses stay inside
// the iteration loop (scalar-cache hits) instead of being hoisted into 2 R L live registers.  Reading the segment
// itself keeps a runtime index away from the by-value argument, which the compiler would then copy to scratch.
typedef const int __attribute__((address_space(4))) wm_kernarg_int;
struct WmTable {
    wm_kernarg_int* t;
    __device__ __forceinline__ int operator[](int k) const { return t[k]; }
};
template <int SEC>
__device__ __forceinline__ WmTable wm_table()
{
    int off = (int)((SEC ? offsetof(WaveMinsumArgs, SZ) : offsetof(WaveMinsumArgs, SX)) / sizeof(int));
    asm volatile("" : "+s"(off));
    return WmTable{(wm_kernarg_int*)__builtin_amdgcn_kernarg_segment_ptr() + off};
}

// sp_minsum_check for the lane's R checks; sb holds their syndrome entries (two bits each: 0, 1, 2 = any other value)
template <int R, int L, bool FREEZE>
__device__ __forceinline__ void wm_check_pass(float (&m)[R][L], uint32_t sb, float alpha, bool act)
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

// sp_minsum_var for the lane's L variables: gathers, the folds from lambda, the inverse rotations.  Returns the
// decisions (bit l: the posterior of variable l is < 0).
template <int R, int L, int SEC, bool LAST, bool FREEZE>
__device__ __forceinline__ uint32_t wm_var_pass(const WaveMinsumArgs& a, float (&m)[R][L], const float (&lamv)[L],
                                                const WmLane& ln, bool act, uint32_t hd_old)
{
    const int P = a.P;
    const WmTable S = wm_table<SEC>();
    uint32_t hd = 0;
#pragma unroll
    for (int l = 0; l < L; ++l) {
        float g[R], o[R];
#pragma unroll
        for (int r = 0; r < R; ++r) g[r] = (r == 0 || l == 0) ? m[r][l] : wm_rot(m[r][l], ln, S[r * L + l]);
        float post = lamv[l];
        if (LAST) {  // the last iteration of the cap: every slot receives the posterior
#pragma unroll
            for (int r = 0; r < R; ++r) post = post + g[r];
#pragma unroll
            for (int r = 0; r < R; ++r) o[r] = post;
        } else {
#pragma unroll
            for (int j = 0; j < R; ++j) {
                float t = post;  // lam + g_0 + ... + g_{j-1}
#pragma unroll
                for (int k = j + 1; k < R; ++k) t = t + g[k];
                o[j] = t;
                post = post + g[j];
            }
        }
        hd |= (uint32_t)(post < 0.0f) << l;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float back = (r == 0 || l == 0) ? o[r] : wm_rot(o[r], ln, P - S[r * L + l]);
            m[r][l] = FREEZE && !act ? m[r][l] : back;
        }
    }
    return FREEZE && !act ? hd_old : hd;
}

// Whether the parities of the lane's R checks over the decisions hd (variable view, bit l) equal their syndrome
// entries; an entry other than 0 / 1 equals no parity
template <int R, int L, int SEC>
__device__ __forceinline__ bool wm_lane_syndrome_ok(const WaveMinsumArgs& a, uint32_t hd, uint32_t sb, const WmLane& ln)
{
    const int P = a.P;
    const WmTable S = wm_table<SEC>();
    bool ok = true;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        uint32_t x = 0;
#pragma unroll
        for (int l = 0; l < L; ++l) {
            const uint32_t h = (r == 0 || l == 0) ? hd : (uint32_t)wm_rot_i((int)hd, ln, P - S[r * L + l]);
            x ^= (h >> l) & 1u;
        }
        ok &= x == ((sb >> (2 * r)) & 3u);
    }
    return ok;
}

template <int R, int L>
__device__ __forceinline__ bool wm_lane_any_inside(const float (&m)[R][L])
{
    bool in = false;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int l = 0; l < L; ++l) in |= wm_inside(m[r][l]);
    return in;
}

// One sector of the wave's syndrome pairs, start to outputs; returns the sector's flag bits and, through itn, its
// iteration count (both per lane, the same on every lane of a group)
template <int R, int L, int SEC, int STOP, bool FREEZE>
__device__ __forceinline__ uint32_t wm_sector(const WaveMinsumArgs& a, const WmLane& ln, long long b, int& itn)
{
    const int P = a.P, n = a.n, N = a.maxIter;
    const int m_s = SEC ? a.mZ : a.mX;
    const int* D = SEC ? a.DZ : a.DX;
    const int* C = SEC ? a.CZ : a.CX;
    const float alpha = a.alpha;

    // syndrome entries of the lane's checks (r, (i + D[r]) mod P): the check update takes their truthiness, the
    // syndrome tests compare them exactly
    uint32_t sb = 0;
    if (ln.live) {
        const uint8_t* s = (SEC ? a.sZ : a.sX) + b * m_s;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint32_t v = s[r * P + wm_wrap(ln.i + D[r], P)];
            sb |= (v > 1u ? 2u : v) << (2 * r);
        }
    }
    // channel LLRs of the lane's variables (l, (i + C[l]) mod P)
    float lamv[L];
#pragma unroll
    for (int l = 0; l < L; ++l) lamv[l] = a.lam;
    if (a.llr != nullptr && ln.live) {
        const float* t = a.llr + (size_t)SEC * n;
#pragma unroll
        for (int l = 0; l < L; ++l) lamv[l] = t[l * P + wm_wrap(ln.i + C[l], P)];
    }
    // every slot starts at its variable's channel LLR; the decisions of N = 0
    float m[R][L];
    uint32_t hd = 0;
    {
        const WmTable S = wm_table<SEC>();
#pragma unroll
        for (int l = 0; l < L; ++l) {
            hd |= (uint32_t)(lamv[l] < 0.0f) << l;
#pragma unroll
            for (int r = 0; r < R; ++r) m[r][l] = lamv[l];
        }
        if (a.llr != nullptr) {  // wave-uniform
#pragma unroll
            for (int l = 1; l < L; ++l)
#pragma unroll
                for (int r = 1; r < R; ++r) m[r][l] = wm_rot(lamv[l], ln, P - S[r * L + l]);
        }
    }

    bool act = ln.live;  // the same on every lane of a group
    bool syn_ok = false; // syndrome stop: the last test of the group's own decisions
    itn = 0;
    for (int it = 0; it < N; ++it) {
        if (__builtin_amdgcn_ballot_w64(act) == 0ull) break;
        itn += act ? 1 : 0;
        wm_check_pass<R, L, FREEZE>(m, sb, alpha, act);
        if (it == N - 1) hd = wm_var_pass<R, L, SEC, true, FREEZE>(a, m, lamv, ln, act, hd);
        else hd = wm_var_pass<R, L, SEC, false, FREEZE>(a, m, lamv, ln, act, hd);
        if (STOP == QEC_STOP_REF && it % 10 == 0) {
            if (wm_group_all(!wm_lane_any_inside<R, L>(m), ln)) act = false;
        } else if (STOP == QEC_STOP_SYNDROME) {
            const bool ok = wm_group_all(wm_lane_syndrome_ok<R, L, SEC>(a, hd, sb, ln), ln);
            syn_ok = act ? ok : syn_ok;
            if (ok) act = false;
        }
    }

    // ---- the final state: flags from the slots and from the decisions, the outputs ----
    const bool convFail = !wm_group_all(!wm_lane_any_inside<R, L>(m), ln);
    if (STOP != QEC_STOP_SYNDROME || N == 0)
        syn_ok = wm_group_all(wm_lane_syndrome_ok<R, L, SEC>(a, hd, sb, ln), ln);
    if (ln.live) {
        uint8_t* e = (SEC ? a.eZ : a.eX) + b * n;
#pragma unroll
        for (int l = 0; l < L; ++l) e[l * P + wm_wrap(ln.i + C[l], P)] = (uint8_t)((hd >> l) & 1u);
        if (a.q != nullptr) {
            float* q = a.q + b * ((long long)(a.mX + a.mZ) * L) + (SEC ? (long long)a.mX * L : 0);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float* row = q + (size_t)(r * P + wm_wrap(ln.i + D[r], P)) * L;
#pragma unroll
                for (int l = 0; l < L; ++l) row[l] = m[r][l];
            }
        }
    }
    uint32_t f = 0;
    if (!syn_ok) f |= SEC ? QEC_SYNDROME_FAIL_Z : QEC_SYNDROME_FAIL_X;
    if (convFail) f |= SEC ? QEC_CONVERGENCE_FAIL_Z : QEC_CONVERGENCE_FAIL_X;
    return f;
}

template <int J, int K, int L, int STOP>
__global__ __launch_bounds__(64) void wave_minsum_kernel(const WaveMinsumArgs a)
{
    const int lane = (int)threadIdx.x, P = a.P, G = a.G;
    const int g = lane / P;  // G for an idle lane
    WmLane ln;
    ln.i = lane - g * P;
    ln.b0 = 4 * lane;
    ln.b1 = ln.b0 + 4 * P;
    ln.gm = (P >= 64 ? ~0ull : ((1ull << P) - 1ull)) << (g * P);
    const long long b = (long long)blockIdx.x * G + g;
    ln.live = g < G && b < a.B;

    uint32_t f;
    int itX, itZ;
    if (STOP != QEC_STOP_FIXED && G > 1) {  // wave-uniform: groups that stop on their own
        f = wm_sector<J, L, 0, STOP, true>(a, ln, b, itX);
        f |= wm_sector<K, L, 1, STOP, true>(a, ln, b, itZ);
    } else {
        f = wm_sector<J, L, 0, STOP, false>(a, ln, b, itX);
        f |= wm_sector<K, L, 1, STOP, false>(a, ln, b, itZ);
    }
    if (ln.live && ln.i == 0) {
        a.flags[b] = (uint8_t)f;
        if (a.iters != nullptr) { a.iters[2 * b] = itX; a.iters[2 * b + 1] = itZ; }
    }
}

// ---- host side ---------------------------------------------------------------
struct WaveMinsumShape {
    int J, K, L;
    const void* fn[3];  // by stop rule
};

template <int J, int K, int L>
static WaveMinsumShape wm_shape()
{
    WaveMinsumShape s{J, K, L, {nullptr, nullptr, nullptr}};
    s.fn[QEC_STOP_REF] = reinterpret_cast<const void*>(&wave_minsum_kernel<J, K, L, QEC_STOP_REF>);
    s.fn[QEC_STOP_FIXED] = reinterpret_cast<const void*>(&wave_minsum_kernel<J, K, L, QEC_STOP_FIXED>);
    s.fn[QEC_STOP_SYNDROME] = reinterpret_cast<const void*>(&wave_minsum_kernel<J, K, L, QEC_STOP_SYNDROME>);
    return s;
}

// the block shapes of bp_decode.hip's runtime-shift variants
static const WaveMinsumShape kWaveMinsumShapes[] = {
    wm_shape<4, 5, 10>(), wm_shape<3, 3, 6>(), wm_shape<2, 3, 6>(), wm_shape<3, 4, 8>(),
    wm_shape<4, 4, 8>(),  wm_shape<3, 5, 10>(), wm_shape<4, 6, 12>(), wm_shape<2, 2, 4>(),
};

// The wave min-sum kernels of a code, or nullptr: a circulant-permutation code with 1 <= P <= 64 and a block shape of
// the table (the limits of bp_decode.hip's select_variant hold for every shape of the table).  No HIP call.
const void* select_wave_minsum(const Code& c)
{
    if (c.general || !c.is_qc || c.P > 64 || c.P < 1) return nullptr;
    if (c.J > kWmMaxR || c.K > kWmMaxR || c.L > kWmMaxL || c.J * c.L > kWmMaxRL || c.K * c.L > kWmMaxRL) return nullptr;
    if ((int)c.EX.size() != c.J * c.L || (int)c.EZ.size() != c.K * c.L) return nullptr;
    for (const WaveMinsumShape& s : kWaveMinsumShapes)
        if (s.J == c.J && s.K == c.K && s.L == c.L) return &s;
    return nullptr;
}

// "wave-minsum J=.. K=.. L=.. P=.. G=.." for qec_decoder_describe
std::string wave_minsum_name(const Code& c)
{
    char buf[96];
    snprintf(buf, sizeof buf, "wave-minsum J=%d K=%d L=%d P=%d G=%d", c.J, c.K, c.L, c.P, 64 / c.P);
    return buf;
}

// One min-sum decode launch in the wave layout: d as launch_decode_sparse's MINSUM kernels read it (minsum = the
// scale, lam, and with prior set llr), no relay tables.  One wave per workgroup, ceil(B / G) workgroups.
int launch_wave_minsum(const void* shape, const Code& c, const SparseDecode& d, hipStream_t stream)
{
    const WaveMinsumShape* s = static_cast<const WaveMinsumShape*>(shape);
    if (d.B <= 0) return QEC_OK;
    if (s == nullptr || s->J != c.J || s->K != c.K || s->L != c.L || c.P < 1 || c.P > 64)
        return fail(QEC_ERR_ARG, "wave min-sum launch: the kernels are another code's");
    if (!d.minsum || d.corr || d.serial || d.gamma != nullptr)
        return fail(QEC_ERR_ARG, "wave min-sum launch: plain min-sum only (no correlated form, serial schedule or relay)");
    if (d.stop < 0 || d.stop > 2) return fail(QEC_ERR_ARG, "wave min-sum launch: unknown stop rule");
    if (d.prior != nullptr && d.llr == nullptr)
        return fail(QEC_ERR_ARG, "wave min-sum launch: min-sum under priors needs its LLR tables");
    WaveMinsumArgs a{};
    a.sX = d.sX; a.sZ = d.sZ; a.eX = d.eX; a.eZ = d.eZ; a.flags = d.flags; a.iters = d.iters; a.q = d.q;
    a.llr = d.prior != nullptr ? d.llr : nullptr;
    a.B = d.B;
    a.P = c.P; a.G = 64 / c.P; a.n = c.n; a.mX = c.mX; a.mZ = c.mZ;
    a.lam = d.lam;
    a.alpha = (float)d.minsum / 256.0f;
    a.maxIter = d.maxIter < 0 ? 0 : d.maxIter;
    wm_relabel(c.EX.data(), c.J, c.L, c.P, a.SX, a.DX, a.CX);
    wm_relabel(c.EZ.data(), c.K, c.L, c.P, a.SZ, a.DZ, a.CZ);
    const long long waves = (d.B + a.G - 1) / a.G;
    if (waves > 0x7fffffffLL) return fail(QEC_ERR_ARG, "wave min-sum launch: batch too large for one launch");
    void* args[] = {&a};
    (void)hipLaunchKernel(s->fn[d.stop], dim3((unsigned)waves), dim3(64), args, 0, stream);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(QEC_ERR_HIP, std::string("wave min-sum launch: ") + hipGetErrorString(err));
    return QEC_OK;
}

}  // namespace qec
