// The wave layout of circulant-permutation codes, shared by the register-resident kernels of bp_wave_minsum.hip and
// bp_wave_relay.hip ("The min-sum form in the wave layout"); the host relabelling is also
// bp_decode.hip's.  HIP translation units only.
//   * one 64-lane wave owns G = 64 / P syndrome pairs, lane g P + i is circulant row i of pair g; the 64 - G P lanes
//     above the groups are idle (they compute on zeros and write nothing).  Sector X is decoded first, then sector Z.
//   * check view: lane i holds, in VGPRs, the message of every edge (r, l, i) of the sector -- check (r, i) <-> variable
//     (l, (E[r][l] + i) mod P) -- for all iterations.  A check's slots in ascending variable order are the column
//     blocks l = 0 .. L-1, so sp_minsum_check's one pass over the row (first minimum, second minimum, argmin on bit
//     patterns, the parity seeded with the syndrome bit, two multiplies by alpha) runs over L registers of the lane.
//   * variable view: lane j holds variable (l, j) of every column l: its channel LLR (L registers, loaded once per
//     sector from the scalar or from the handle's table) and, during a column's update, its R incoming messages,
//     gathered by the block rotations (ds_bpermute_b32).  A variable's messages in ascending check order are the row
//     blocks r = 0 .. R-1, so the variable passes' left folds run as they stand; the outputs go back with the inverse
//     rotations.
//   * relabel() makes the blocks of row 0 and column 0 rotation-free.
// Control flow stays wave-uniform: every lane executes every pass, and a finished group's registers are kept by
// selects (FREEZE), so a permute never runs with part of a group's lanes disabled.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "qec_internal.h"

#pragma clang fp contract(off)

namespace qec {

// ---- lane relabelling ------------------------------------------------------
// Block (r, l) of a sector is the circulant "check (r, i) <-> variable (l, (E[r][l] + i) mod P)".
// Storing check (r, i) in lane (i - D[r]) mod P and variable (l, j) in lane (j - C[l]) mod P
// turns the block's check->variable lane rotation into S[r][l] = (E[r][l] + D[r] - C[l]) mod P.
// With C[l] = E[0][l] and D[r] = (C[0] - E[r][0]) mod P the R + L - 1 blocks of row 0 and
// column 0 need no rotation at all (a spanning tree of the block graph), so those edges skip
// the ds_bpermute in both directions.  Arithmetic (and so every output bit) is unchanged.
inline void relabel(const int* E, int R, int L, int P, bool on, int* S, int* D, int* C)
{
    if (!on) {
        for (int k = 0; k < R * L; ++k) S[k] = E[k];
        for (int r = 0; r < R; ++r) D[r] = 0;
        for (int l = 0; l < L; ++l) C[l] = 0;
        return;
    }
    for (int l = 0; l < L; ++l) C[l] = E[l];
    for (int r = 0; r < R; ++r) D[r] = ((C[0] - E[r * L]) % P + P) % P;
    for (int r = 0; r < R; ++r)
        for (int l = 0; l < L; ++l) S[r * L + l] = ((E[r * L + l] + D[r] - C[l]) % P + P) % P;
}

// ---- device side: the lane helpers of the register-resident kernels ---------
constexpr int kWaveMaxR = 6, kWaveMaxL = 12, kWaveMaxRL = 72;  // the largest shape of the wave kernels, (4,6,12)

struct WaveLane {
    int i;       // in-group index (an idle lane: its index above the last group)
    int b0, b1;  // bpermute bases 4 (gb + i) and 4 (gb + i + P)
    unsigned long long gm;   // the lanes of this lane's group
    unsigned long long gm0;  // the lanes of group 0 (wave-uniform; the relay kernels only)
    bool live;   // the lane belongs to a syndrome pair of the batch
};

// The value of lane gb + (i - s) mod P of this lane's group, s in [0, P] (0 and P: the lane's own).  ds_bpermute
// selects lane (addr >> 2) & 63; the +256 keeps the address non-negative.
__device__ __forceinline__ int wave_rot_i(int v, const WaveLane& ln, int s)
{
    const int base = ln.i < s ? ln.b1 : ln.b0;
    return __builtin_amdgcn_ds_bpermute(base + (256 - 4 * s), v);
}
__device__ __forceinline__ float wave_rot(float v, const WaveLane& ln, int s)
{
    return __int_as_float(wave_rot_i(__float_as_int(v), ln, s));
}
__device__ __forceinline__ int wave_wrap(int x, int P) { return x >= P ? x - P : x; }
// Whether pred holds on every lane of the lane's group (OWN), or of group 0: wave-uniform, for one group per wave
template <bool OWN>
__device__ __forceinline__ bool wave_group_all(bool pred, const WaveLane& ln)
{
    return (__builtin_amdgcn_ballot_w64(!pred) & (OWN ? ln.gm : ln.gm0)) == 0ull;
}
__device__ __forceinline__ bool wave_inside(float x) { return __builtin_fabsf(x) < kMinSumInside; }

// The sector's shift table of argument struct A, read from the kernel-argument segment (the kernel's one argument
// starts at its offset 0) behind an offset laundered once per use (it is 0), so that the R L shift loads and rotation
// addresses stay inside the iteration loop (scalar-cache hits) instead of being hoisted into 2 R L live registers.
// Reading the segment itself keeps a runtime index away from the by-value argument, which the compiler would then
// copy to scratch.
typedef const int __attribute__((address_space(4))) wave_kernarg_int;
struct WaveTable {
    wave_kernarg_int* t;
    __device__ __forceinline__ int operator[](int k) const { return t[k]; }
};
template <class A, int SEC>
__device__ __forceinline__ WaveTable wave_table()
{
    int off = (int)((SEC ? offsetof(A, SZ) : offsetof(A, SX)) / sizeof(int));
    asm volatile("" : "+s"(off));
    return WaveTable{(wave_kernarg_int*)__builtin_amdgcn_kernarg_segment_ptr() + off};
}

// The syndrome entries of the lane's checks (r, (i + D[r]) mod P) of pair b, two bits each: 0, 1, 2 = any other
// value.  The check update takes their truthiness, the syndrome tests compare them exactly.
template <int R, int SEC, class A>
__device__ __forceinline__ uint32_t wave_load_syndrome(const A& a, const WaveLane& ln, long long b)
{
    const int P = a.P;
    const int m_s = SEC ? a.mZ : a.mX;
    const int* D = SEC ? a.DZ : a.DX;
    uint32_t sb = 0;
    if (ln.live) {
        const uint8_t* s = (SEC ? a.sZ : a.sX) + b * m_s;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint32_t v = s[r * P + wave_wrap(ln.i + D[r], P)];
            sb |= (v > 1u ? 2u : v) << (2 * r);
        }
    }
    return sb;
}

// sp_minsum_check (bp_sparse.hip) for the lane's R checks; sb as wave_load_syndrome's
template <int R, int L, bool FREEZE>
__device__ __forceinline__ void wave_check_pass(float (&m)[R][L], uint32_t sb, float alpha, bool act)
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

// wave_check_pass for one row of the lane's checks (the layered kernels: a layer is a block row): m holds the row's L
// inputs and receives its L outputs; t = the syndrome entry is non-zero
template <int L>
__device__ __forceinline__ void wave_check_row(float (&m)[L], bool t, float alpha)
{
    uint32_t min1 = kMinSumCap, min2 = kMinSumCap;
    uint32_t sgn = t ? 0x80000000u : 0u;  // the parity, kept in the sign position
    int arg = -1;
#pragma unroll
    for (int l = 0; l < L; ++l) {
        const uint32_t b = __float_as_uint(m[l]);
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
        const uint32_t b = __float_as_uint(m[l]);
        m[l] = __uint_as_float((l == arg ? o2 : o1) | ((sgn ^ b) & 0x80000000u));
    }
}

// ---- the soft-syndrome form (qec_decoder_set_syndrome_priors): SOFT siblings -----------------
// The channel LLRs of the measurement-error variables of the lane's checks, at the index where wave_load_syndrome reads
// the syndrome byte; mu = the sector's table.  An idle lane computes on +0.0f.
template <int R, int SEC, class A>
__device__ __forceinline__ void wave_load_mu(float (&muv)[R], const A& a, const float* __restrict__ mu, const WaveLane& ln)
{
    const int P = a.P;
    const int* D = SEC ? a.DZ : a.DX;
#pragma unroll
    for (int r = 0; r < R; ++r) muv[r] = 0.0f;
    if (ln.live) {
#pragma unroll
        for (int r = 0; r < R; ++r) muv[r] = mu[r * P + wave_wrap(ln.i + D[r], P)];
    }
}

// The virtual input of a row: it enters the minima and the parity ahead of the L registers (the outputs do not depend
// on an input's position); virt = it holds the first minimum so far
__device__ __forceinline__ void wave_soft_input(float mu, uint32_t& min1, uint32_t& sgn, bool& virt)
{
    const uint32_t b = __float_as_uint(mu);
    const uint32_t x = b & 0x7FFFFFFFu;
    sgn ^= b;
    virt = x < kMinSumCap;
    min1 = virt ? x : kMinSumCap;
}
// The row's measurement decision f = mu + rho < 0, rho = the virtual slot's own output: o2 where the virtual input is
// the first minimum (arg never moved), else o1, under the parity without the input's own sign
__device__ __forceinline__ bool wave_soft_decision(float mu, uint32_t o1, uint32_t o2, uint32_t sgn, bool virt, int arg)
{
    const uint32_t b = __float_as_uint(mu);
    const float rho = __uint_as_float(((virt && arg < 0) ? o2 : o1) | ((sgn ^ b) & 0x80000000u));
    const float postm = mu + rho;
    return postm < 0.0f;
}

// wave_check_pass with the virtual inputs muv; returns the decisions f of the lane's R checks (bit r), a frozen
// group's kept
template <int R, int L, bool FREEZE>
__device__ __forceinline__ uint32_t wave_check_pass_soft(float (&m)[R][L], uint32_t sb, const float (&muv)[R], float alpha,
                                                         bool act, uint32_t fb_old)
{
    uint32_t fb = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        uint32_t min1, min2 = kMinSumCap;
        uint32_t sgn = ((sb >> (2 * r)) & 3u) != 0u ? 0x80000000u : 0u;  // the parity, kept in the sign position
        bool virt;
        wave_soft_input(muv[r], min1, sgn, virt);
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
        fb |= (uint32_t)wave_soft_decision(muv[r], o1, o2, sgn, virt, arg) << r;
    }
    return FREEZE && !act ? fb_old : fb;
}

// wave_check_row with the virtual input mu; returns the row's decision f
template <int L>
__device__ __forceinline__ bool wave_check_row_soft(float (&m)[L], bool t, float mu, float alpha)
{
    uint32_t min1, min2 = kMinSumCap;
    uint32_t sgn = t ? 0x80000000u : 0u;  // the parity, kept in the sign position
    bool virt;
    wave_soft_input(mu, min1, sgn, virt);
    int arg = -1;
#pragma unroll
    for (int l = 0; l < L; ++l) {
        const uint32_t b = __float_as_uint(m[l]);
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
        const uint32_t b = __float_as_uint(m[l]);
        m[l] = __uint_as_float((l == arg ? o2 : o1) | ((sgn ^ b) & 0x80000000u));
    }
    return wave_soft_decision(mu, o1, o2, sgn, virt, arg);
}

// wave_lane_syndrome_ok with the lane's decisions f (bit r) XORed into the parities.  SEC picks the shift table of
// argument struct A, which sits at offset 0 of the kernel's argument.
template <int R, int L, int SEC, class A>
__device__ __forceinline__ bool wave_lane_syndrome_ok_soft(const A& a, uint32_t hd, uint32_t sb, uint32_t fb,
                                                           const WaveLane& ln)
{
    const int P = a.P;
    const WaveTable S = wave_table<A, SEC>();
    bool ok = true;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        uint32_t x = (fb >> r) & 1u;
#pragma unroll
        for (int l = 0; l < L; ++l) {
            const uint32_t h = (r == 0 || l == 0) ? hd : (uint32_t)wave_rot_i((int)hd, ln, P - S[r * L + l]);
            x ^= (h >> l) & 1u;
        }
        ok &= x == ((sb >> (2 * r)) & 3u);
    }
    return ok;
}

// The decisions f of the lane's checks of pair b out (live lanes; fo = the sector's array, m_s its checks per pair)
template <int R, int SEC, class A>
__device__ __forceinline__ void wave_store_flips(const A& a, uint8_t* __restrict__ fo, const WaveLane& ln, long long b,
                                                 uint32_t fb)
{
    const int P = a.P;
    const int m_s = SEC ? a.mZ : a.mX;
    const int* D = SEC ? a.DZ : a.DX;
    if (ln.live) {
        uint8_t* f = fo + b * m_s;
#pragma unroll
        for (int r = 0; r < R; ++r) f[r * P + wave_wrap(ln.i + D[r], P)] = (uint8_t)((fb >> r) & 1u);
    }
}

// Whether the parities of the lane's R checks over the decisions hd (variable view, bit l) equal their syndrome
// entries; an entry other than 0 / 1 equals no parity
template <int R, int L, int SEC, class A>
__device__ __forceinline__ bool wave_lane_syndrome_ok(const A& a, uint32_t hd, uint32_t sb, const WaveLane& ln)
{
    const int P = a.P;
    const WaveTable S = wave_table<A, SEC>();
    bool ok = true;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        uint32_t x = 0;
#pragma unroll
        for (int l = 0; l < L; ++l) {
            const uint32_t h = (r == 0 || l == 0) ? hd : (uint32_t)wave_rot_i((int)hd, ln, P - S[r * L + l]);
            x ^= (h >> l) & 1u;
        }
        ok &= x == ((sb >> (2 * r)) & 3u);
    }
    return ok;
}

template <int R, int L>
__device__ __forceinline__ bool wave_lane_any_inside(const float (&m)[R][L])
{
    bool in = false;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int l = 0; l < L; ++l) in |= wave_inside(m[r][l]);
    return in;
}

// The gather of a variable pass: the lane's variable of column l receives its R incoming messages, by the block
// rotations.  (The folds, the scatter, the LLR load and the output stores stay in the two files: shared helpers for
// them changed the kernels' instruction streams)
template <int R, int L>
__device__ __forceinline__ void wave_gather(float (&g)[R], const float (&m)[R][L], int l, const WaveLane& ln,
                                            const WaveTable& S)
{
#pragma unroll
    for (int r = 0; r < R; ++r) g[r] = (r == 0 || l == 0) ? m[r][l] : wave_rot(m[r][l], ln, S[r * L + l]);
}

// The lane's place in the wave of workgroup blockIdx.x, and through b its syndrome pair.  ln is an out-parameter: the
// same function returning the struct by value changed every kernel's instruction stream.
template <class A>
__device__ __forceinline__ void wave_lane(const A& a, WaveLane& ln, long long& b)
{
    const int lane = (int)threadIdx.x, P = a.P, G = a.G;
    const int g = lane / P;  // G for an idle lane
    ln.i = lane - g * P;
    ln.b0 = 4 * lane;
    ln.b1 = ln.b0 + 4 * P;
    ln.gm0 = P >= 64 ? ~0ull : ((1ull << P) - 1ull);
    ln.gm = ln.gm0 << (g * P);
    b = (long long)blockIdx.x * G + g;
    ln.live = g < G && b < a.B;
}
// The pair's flags byte and iteration counts, by the first lane of its group
template <class A>
__device__ __forceinline__ void wave_store_flags(const A& a, const WaveLane& ln, long long b, uint32_t f, int itX,
                                                 int itZ)
{
    if (ln.live && ln.i == 0) {
        a.flags[b] = (uint8_t)f;
        if (a.iters != nullptr) { a.iters[2 * b] = itX; a.iters[2 * b + 1] = itZ; }
    }
}

// ---- host side: the shape table, the shared argument fields, the launch -----
struct WaveShape {
    int J, K, L;
    const void* fn[3];  // by stop rule
};

// The block shapes of bp_decode.hip's runtime-shift variants, as a table of f<J, K, L>()
#define QEC_WAVE_SHAPE_TABLE(f) \
    f<4, 5, 10>(), f<3, 3, 6>(), f<2, 3, 6>(), f<3, 4, 8>(), f<4, 4, 8>(), f<3, 5, 10>(), f<4, 6, 12>(), f<2, 2, 4>()

// The row of a shape table for a code, or nullptr: a circulant-permutation code with 1 <= P <= 64 and a block shape of
// the table (the limits of bp_decode.hip's select_variant hold for every shape of the table).  No HIP call.
template <size_t N>
inline const WaveShape* wave_find_shape(const WaveShape (&shapes)[N], const Code& c)
{
    if (c.general || !c.is_qc || c.P > 64 || c.P < 1) return nullptr;
    if (c.J > kWaveMaxR || c.K > kWaveMaxR || c.L > kWaveMaxL || c.J * c.L > kWaveMaxRL || c.K * c.L > kWaveMaxRL)
        return nullptr;
    if ((int)c.EX.size() != c.J * c.L || (int)c.EZ.size() != c.K * c.L) return nullptr;
    for (const WaveShape& s : shapes)
        if (s.J == c.J && s.K == c.K && s.L == c.L) return &s;
    return nullptr;
}

// "wave-<kind> J=.. K=.. L=.. P=.. G=.." for qec_decoder_describe
inline std::string wave_name(const char* kind, const Code& c)
{
    return std::string("wave-") + kind + " J=" + std::to_string(c.J) + " K=" + std::to_string(c.K) +
           " L=" + std::to_string(c.L) + " P=" + std::to_string(c.P) + " G=" + std::to_string(64 / c.P);
}

// Whether the launcher was handed the row of its own table that select found for this code
inline bool wave_shape_fits(const WaveShape* s, const Code& c)
{
    return s != nullptr && s->J == c.J && s->K == c.K && s->L == c.L && c.P >= 1 && c.P <= 64;
}

// The fields that the argument structs of both kernel families share, from d as launch_decode_sparse's MINSUM kernels
// read it (minsum = the scale, lam, and with prior set llr), after the checks of what is read here.  `who` starts the
// error texts.
template <class A>
inline int wave_fill_args(const char* who, A& a, const Code& c, const SparseDecode& d)
{
    if (d.stop < 0 || d.stop > 2) return fail(QEC_ERR_ARG, std::string(who) + ": unknown stop rule");
    if (d.prior != nullptr && d.llr == nullptr)
        return fail(QEC_ERR_ARG, std::string(who) + ": min-sum under priors needs its LLR tables");
    a.sX = d.sX; a.sZ = d.sZ; a.eX = d.eX; a.eZ = d.eZ; a.flags = d.flags; a.iters = d.iters; a.q = d.q;
    a.llr = d.prior != nullptr ? d.llr : nullptr;
    a.B = d.B;
    a.P = c.P; a.G = 64 / c.P; a.n = c.n; a.mX = c.mX; a.mZ = c.mZ;
    a.lam = d.lam;
    a.alpha = (float)d.minsum / 256.0f;
    a.maxIter = d.maxIter < 0 ? 0 : d.maxIter;
    relabel(c.EX.data(), c.J, c.L, c.P, true, a.SX, a.DX, a.CX);
    relabel(c.EZ.data(), c.K, c.L, c.P, true, a.SZ, a.DZ, a.CZ);
    return QEC_OK;
}

// One wave per workgroup, ceil(B / G) workgroups
template <class A>
inline int wave_launch(const char* who, const void* fn, A& a, hipStream_t stream)
{
    const long long waves = (a.B + a.G - 1) / a.G;
    if (waves > 0x7fffffffLL) return fail(QEC_ERR_ARG, std::string(who) + ": batch too large for one launch");
    void* args[] = {&a};
    (void)hipLaunchKernel(fn, dim3((unsigned)waves), dim3(64), args, 0, stream);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(QEC_ERR_HIP, std::string(who) + ": " + hipGetErrorString(err));
    return QEC_OK;
}

// wave_launch for an argument struct that wraps the shared fields (B pairs, G per wave)
template <class A>
inline int wave_launch_as(const char* who, const void* fn, A& a, long long B, int G, hipStream_t stream)
{
    const long long waves = (B + G - 1) / G;
    if (waves > 0x7fffffffLL) return fail(QEC_ERR_ARG, std::string(who) + ": batch too large for one launch");
    void* args[] = {&a};
    (void)hipLaunchKernel(fn, dim3((unsigned)waves), dim3(64), args, 0, stream);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(QEC_ERR_HIP, std::string(who) + ": " + hipGetErrorString(err));
    return QEC_OK;
}

}  // namespace qec
