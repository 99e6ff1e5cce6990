// Register-resident Relay-BP for circulant-permutation codes (QEC_OPT_RELAY_WAVE; DESIGN.md section 2, "The relay form
// in the wave layout").  The rule is sp_relay_decode's (bp_sparse.hip) in every bit; the layout, the lane
// helpers, the check pass, the syndrome test and the host-side shape table, argument filling and launch are qec_wave.h's,
// shared with bp_wave_minsum.hip.  This file holds what is the relay's own: the argument struct, sp_relay_var's pass
// (bias, memory, the `last` select), the group sum, the slots at the start of a leg, the sector function and the kernel:
//   * check view: the R L slots of the lane's checks in VGPRs.  Variable view: per column l the channel LLR, the
//     relay's memory M and one decision bit, all in VGPRs.
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

#include <cstdint>
#include <string>

#include "qec_internal.h"
#include "qec_wave.h"

#pragma clang fp contract(off)

namespace qec {

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
    // lane-relabelled circulant tables (relabel, qec_wave.h)
    int SX[kWaveMaxRL], SZ[kWaveMaxRL];  // rotation of block (r, l) between check and variable views
    int DX[kWaveMaxR], DZ[kWaveMaxR];    // check-view lane lambda holds check (r, (lambda + D[r]) mod P)
    int CX[kWaveMaxL], CZ[kWaveMaxL];    // var-view lane mu holds variable (l, (mu + C[l]) mod P)
};

// sp_relay_var for the lane's L variables in leg `leg`: the gamma loads, the bias, the gathers, the folds from the
// bias, M = the posterior, the inverse rotations.  `last` (per lane: the group's iteration N - 1 of its leg) gives every
// slot the posterior -- the fold that ends the extrinsic pass -- by select.  Returns the decisions (bit l).
template <int R, int L, int SEC, bool FREEZE>
__device__ __forceinline__ uint32_t wr_var_pass(const WaveRelayArgs& a, float (&m)[R][L], const float (&lamv)[L],
                                                float (&mem)[L], const WaveLane& ln, bool act, bool last, int leg,
                                                uint32_t hd_old)
{
    const int P = a.P;
    const int* C = SEC ? a.CZ : a.CX;
    const WaveTable S = wave_table<WaveRelayArgs, SEC>();
    float gam[L];
#pragma unroll
    for (int l = 0; l < L; ++l) gam[l] = 0.0f;
    if (ln.live) {  // the permutes below run with EXEC full again
        const float* t = a.gamma + ((size_t)leg * 2 + SEC) * (size_t)a.n;
#pragma unroll
        for (int l = 0; l < L; ++l) gam[l] = t[l * P + wave_wrap(ln.i + C[l], P)];
    }
    uint32_t hd = 0;
#pragma unroll
    for (int l = 0; l < L; ++l) {
        float g[R], o[R];
        wave_gather<R, L>(g, m, l, ln, S);
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
            const float back = (r == 0 || l == 0) ? out : wave_rot(out, ln, P - S[r * L + l]);
            m[r][l] = FREEZE && !act ? m[r][l] : back;
        }
    }
    return FREEZE && !act ? hd_old : hd;
}

// The sum over the lanes of the lane's group of x, modulo 2^32, from BITS ballots: bit j of the sum's terms is set on
// popcount(ballot & group) lanes.  Integer adds, so the order does not matter; x < 2^BITS on every lane.
template <int BITS, bool FREEZE>
__device__ __forceinline__ uint32_t wr_group_sum(uint32_t x, const WaveLane& ln)
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
                                              const WaveLane& ln, bool sel)
{
    const int P = a.P;
    const WaveTable S = wave_table<WaveRelayArgs, SEC>();
    if (a.llr != nullptr) {  // wave-uniform
#pragma unroll
        for (int l = 0; l < L; ++l)
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float x = (r == 0 || l == 0) ? lamv[l] : wave_rot(lamv[l], ln, P - S[r * L + l]);
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
__device__ __forceinline__ uint32_t wr_sector(const WaveRelayArgs& a, const WaveLane& ln, long long b, int& itn)
{
    const int P = a.P, n = a.n, N = a.maxIter;
    const int legs = a.legs, sols_max = a.solutions;
    const int* D = SEC ? a.DZ : a.DX;
    const int* C = SEC ? a.CZ : a.CX;
    const float alpha = a.alpha;
    const bool weigh = sols_max > 1;  // wave-uniform

    const uint32_t sb = wave_load_syndrome<R, SEC>(a, ln, b);
    // channel LLRs of the lane's variables (l, (i + C[l]) mod P); leg 0: M = lambda, the decisions of N = 0
    float lamv[L], mem[L];
#pragma unroll
    for (int l = 0; l < L; ++l) lamv[l] = a.lam;
    if (a.llr != nullptr && ln.live) {
        const float* t = a.llr + (size_t)SEC * n;
#pragma unroll
        for (int l = 0; l < L; ++l) lamv[l] = t[l * P + wave_wrap(ln.i + C[l], P)];
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
            wave_check_pass<R, L, FREEZE>(m, sb, alpha, act);
            hd = wr_var_pass<R, L, SEC, FREEZE>(a, m, lamv, mem, ln, act, last, leg, hd);
            k += act ? 1 : 0;
        }
        // which groups end their leg here (the call's stop rule, counted within the leg)
        bool end = act && k == N;
        if (STOP == QEC_STOP_REF && N > 0) {
            const bool t = act && (k - 1) % 10 == 0;
            if (__builtin_amdgcn_ballot_w64(t) != 0ull) {
                const bool out = wave_group_all<FREEZE>(!wave_lane_any_inside<R, L>(m), ln);
                if (t && out) end = true;
            }
        } else if (STOP == QEC_STOP_SYNDROME && N > 0) {
            bad = !wave_group_all<FREEZE>(wave_lane_syndrome_ok<R, L, SEC>(a, hd, sb, ln), ln);
            if (act && !bad) end = true;
        }
        if (__builtin_amdgcn_ballot_w64(end) == 0ull) continue;

        // ---- the end of a leg: a solution?  the next leg, or the end of the group's relay ----
        if (STOP != QEC_STOP_SYNDROME || N == 0)
            bad = !wave_group_all<FREEZE>(wave_lane_syndrome_ok<R, L, SEC>(a, hd, sb, ln), ln);
        const bool solved = end && !bad;
        uint32_t W = 0u;
        if (weigh && __builtin_amdgcn_ballot_w64(solved) != 0ull) {
            if (a.weight != nullptr) {
                uint32_t x = 0u;
                if (ln.live) {
                    const int32_t* w = a.weight + (size_t)SEC * n;
#pragma unroll
                    for (int l = 0; l < L; ++l)
                        x += ((hd >> l) & 1u) ? (uint32_t)w[l * P + wave_wrap(ln.i + C[l], P)] : 0u;
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
    const bool convFail = !wave_group_all<FREEZE>(!wave_lane_any_inside<R, L>(m), ln);
    if (ln.live) {
        const uint32_t h = sols ? best : hd;
        uint8_t* e = (SEC ? a.eZ : a.eX) + b * n;
#pragma unroll
        for (int l = 0; l < L; ++l) e[l * P + wave_wrap(ln.i + C[l], P)] = (uint8_t)((h >> l) & 1u);
        if (a.q != nullptr) {
            float* q = a.q + b * ((long long)(a.mX + a.mZ) * L) + (SEC ? (long long)a.mX * L : 0);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float* row = q + (size_t)(r * P + wave_wrap(ln.i + D[r], P)) * L;
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
    long long b;
    WaveLane ln;
    wave_lane(a, ln, b);

    uint32_t f;
    int itX, itZ;
    if (a.G > 1) {  // wave-uniform: groups that finish on their own, under every stop rule
        f = wr_sector<J, L, 0, STOP, true>(a, ln, b, itX);
        f |= wr_sector<K, L, 1, STOP, true>(a, ln, b, itZ);
    } else {
        f = wr_sector<J, L, 0, STOP, false>(a, ln, b, itX);
        f |= wr_sector<K, L, 1, STOP, false>(a, ln, b, itZ);
    }
    wave_store_flags(a, ln, b, f, itX, itZ);
}

// ---- host side ---------------------------------------------------------------
template <int J, int K, int L>
static WaveShape wr_shape()
{
    WaveShape s{J, K, L, {nullptr, nullptr, nullptr}};
    s.fn[QEC_STOP_REF] = reinterpret_cast<const void*>(&wave_relay_kernel<J, K, L, QEC_STOP_REF>);
    s.fn[QEC_STOP_FIXED] = reinterpret_cast<const void*>(&wave_relay_kernel<J, K, L, QEC_STOP_FIXED>);
    s.fn[QEC_STOP_SYNDROME] = reinterpret_cast<const void*>(&wave_relay_kernel<J, K, L, QEC_STOP_SYNDROME>);
    return s;
}

static const WaveShape kWaveRelayShapes[] = {QEC_WAVE_SHAPE_TABLE(wr_shape)};

// The wave relay kernels of a code, or nullptr: the codes of select_wave_minsum (wave_find_shape).  No HIP call.
const void* select_wave_relay(const Code& c) { return wave_find_shape(kWaveRelayShapes, c); }

std::string wave_relay_name(const Code& c) { return wave_name("relay", c); }

// One relay decode launch in the wave layout: d as launch_decode_sparse's RELAY kernels read it (minsum = the scale,
// lam, with prior set llr, gamma = the tables, legs, solutions, relay_weight).  It allocates nothing.
int launch_wave_relay(const void* shape, const Code& c, const SparseDecode& d, hipStream_t stream)
{
    const char* who = "wave relay launch";
    const WaveShape* s = static_cast<const WaveShape*>(shape);
    if (d.B <= 0) return QEC_OK;
    if (!wave_shape_fits(s, c)) return fail(QEC_ERR_ARG, "wave relay launch: the kernels are another code's");
    if (!d.minsum || d.gamma == nullptr || d.corr || d.serial)
        return fail(QEC_ERR_ARG, "wave relay launch: min-sum with relay tables only (no correlated form or serial schedule)");
    if (d.legs < 1 || d.legs > kRelayMaxLegs || d.solutions < 1 || d.solutions > kRelayMaxSolutions)
        return fail(QEC_ERR_ARG, "wave relay launch: the relay needs its tables (qec_decoder_set_relay)");
    WaveRelayArgs a{};
    const int rc = wave_fill_args(who, a, c, d);
    if (rc != QEC_OK) return rc;
    a.gamma = d.gamma;
    a.weight = d.relay_weight;
    a.legs = d.legs;
    a.solutions = d.solutions;
    return wave_launch(who, s->fn[d.stop], a, stream);
}

}  // namespace qec
