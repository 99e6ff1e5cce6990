// Register-resident scaled min-sum for circulant-permutation codes (QEC_OPT_MINSUM_WAVE; DESIGN.md section 2,
// "The min-sum form in the wave layout").  The rule is sp_minsum_decode's (bp_sparse.hip) in every bit; the layout,
// the lane helpers, the check pass, the syndrome test and the host-side shape table, argument filling and launch are
// qec_wave.h's.  This file holds what is min-sum's own: the argument struct, sp_minsum_var's folds from lambda (with
// the LAST form of the cap's last iteration), the sector function and the kernel -- and, behind them, the same for
// layered min-sum (QEC_OPT_MINSUM_SCHEDULE = 1): wl_sector and wave_layered_kernel over the same argument struct.
// No LDS beyond the permutes' crossbar, no atomics, no barriers, no scratch.  Every loop is bounded by maxIter.
//
// Groups of one wave stop on their own (G > 1, reference and syndrome stop): control flow stays wave-uniform, every
// lane executes every pass, and a finished group's registers (messages, decisions, count) are kept by selects, so a
// permute never runs with part of a group's lanes disabled.  The wave leaves the loop when no live group runs.  With
// G = 1 or under the fixed stop nothing is ever frozen and the selects are not compiled in (a wave-uniform branch
// on G picks the body).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "qec_internal.h"
#include "qec_wave.h"

#pragma clang fp contract(off)

namespace qec {

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
    // lane-relabelled circulant tables (relabel, qec_wave.h)
    int SX[kWaveMaxRL], SZ[kWaveMaxRL];  // rotation of block (r, l) between check and variable views
    int DX[kWaveMaxR], DZ[kWaveMaxR];    // check-view lane lambda holds check (r, (lambda + D[r]) mod P)
    int CX[kWaveMaxL], CZ[kWaveMaxL];    // var-view lane mu holds variable (l, (mu + C[l]) mod P)
};

// The argument of the SOFT kernels (syndrome priors; DESIGN.md section 2, "The soft-syndrome form"): the plain kernels'
// block at offset 0, so that wave_table and every helper read it as they stand, and behind it the table and the outputs
struct WaveSoftArgs {
    WaveMinsumArgs w;
    const float* mu;     // the channel LLRs of the measurement-error variables, sector X [mX] then Z [mZ]
    uint8_t* fX;         // nullable: [B][mX] measurement decisions out
    uint8_t* fZ;         // nullable: [B][mZ]
};

// sp_minsum_var for the lane's L variables: gathers, the folds from lambda, the inverse rotations.  Returns the
// decisions (bit l: the posterior of variable l is < 0).
template <int R, int L, int SEC, bool LAST, bool FREEZE>
__device__ __forceinline__ uint32_t wm_var_pass(const WaveMinsumArgs& a, float (&m)[R][L], const float (&lamv)[L],
                                                const WaveLane& ln, bool act, uint32_t hd_old)
{
    const int P = a.P;
    const WaveTable S = wave_table<WaveMinsumArgs, SEC>();
    uint32_t hd = 0;
#pragma unroll
    for (int l = 0; l < L; ++l) {
        float g[R], o[R];
        wave_gather<R, L>(g, m, l, ln, S);
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
            const float back = (r == 0 || l == 0) ? o[r] : wave_rot(o[r], ln, P - S[r * L + l]);
            m[r][l] = FREEZE && !act ? m[r][l] : back;
        }
    }
    return FREEZE && !act ? hd_old : hd;
}

// One sector of the wave's syndrome pairs, start to outputs; returns the sector's flag bits and, through itn, its
// iteration count (both per lane, the same on every lane of a group)
template <int R, int L, int SEC, int STOP, bool FREEZE>
__device__ __forceinline__ uint32_t wm_sector(const WaveMinsumArgs& a, const WaveLane& ln, long long b, int& itn)
{
    const int P = a.P, n = a.n, N = a.maxIter;
    const int* D = SEC ? a.DZ : a.DX;
    const int* C = SEC ? a.CZ : a.CX;
    const float alpha = a.alpha;

    const uint32_t sb = wave_load_syndrome<R, SEC>(a, ln, b);
    // channel LLRs of the lane's variables (l, (i + C[l]) mod P)
    float lamv[L];
#pragma unroll
    for (int l = 0; l < L; ++l) lamv[l] = a.lam;
    if (a.llr != nullptr && ln.live) {
        const float* t = a.llr + (size_t)SEC * n;
#pragma unroll
        for (int l = 0; l < L; ++l) lamv[l] = t[l * P + wave_wrap(ln.i + C[l], P)];
    }
    // every slot starts at its variable's channel LLR; the decisions of N = 0
    float m[R][L];
    uint32_t hd = 0;
    {
        const WaveTable S = wave_table<WaveMinsumArgs, SEC>();
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
                for (int r = 1; r < R; ++r) m[r][l] = wave_rot(lamv[l], ln, P - S[r * L + l]);
        }
    }

    bool act = ln.live;  // the same on every lane of a group
    bool syn_ok = false; // syndrome stop: the last test of the group's own decisions
    itn = 0;
    for (int it = 0; it < N; ++it) {
        if (__builtin_amdgcn_ballot_w64(act) == 0ull) break;
        itn += act ? 1 : 0;
        wave_check_pass<R, L, FREEZE>(m, sb, alpha, act);
        if (it == N - 1) hd = wm_var_pass<R, L, SEC, true, FREEZE>(a, m, lamv, ln, act, hd);
        else hd = wm_var_pass<R, L, SEC, false, FREEZE>(a, m, lamv, ln, act, hd);
        if (STOP == QEC_STOP_REF && it % 10 == 0) {
            if (wave_group_all<true>(!wave_lane_any_inside<R, L>(m), ln)) act = false;
        } else if (STOP == QEC_STOP_SYNDROME) {
            const bool ok = wave_group_all<true>(wave_lane_syndrome_ok<R, L, SEC>(a, hd, sb, ln), ln);
            syn_ok = act ? ok : syn_ok;
            if (ok) act = false;
        }
    }

    // ---- the final state: flags from the slots and from the decisions, the outputs ----
    const bool convFail = !wave_group_all<true>(!wave_lane_any_inside<R, L>(m), ln);
    if (STOP != QEC_STOP_SYNDROME || N == 0)
        syn_ok = wave_group_all<true>(wave_lane_syndrome_ok<R, L, SEC>(a, hd, sb, ln), ln);
    if (ln.live) {
        uint8_t* e = (SEC ? a.eZ : a.eX) + b * n;
#pragma unroll
        for (int l = 0; l < L; ++l) e[l * P + wave_wrap(ln.i + C[l], P)] = (uint8_t)((hd >> l) & 1u);
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
    if (!syn_ok) f |= SEC ? QEC_SYNDROME_FAIL_Z : QEC_SYNDROME_FAIL_X;
    if (convFail) f |= SEC ? QEC_CONVERGENCE_FAIL_Z : QEC_CONVERGENCE_FAIL_X;
    return f;
}

template <int J, int K, int L, int STOP>
__global__ __launch_bounds__(64) void wave_minsum_kernel(const WaveMinsumArgs a)
{
    long long b;
    WaveLane ln;
    wave_lane(a, ln, b);

    uint32_t f;
    int itX, itZ;
    if (STOP != QEC_STOP_FIXED && a.G > 1) {  // wave-uniform: groups that stop on their own
        f = wm_sector<J, L, 0, STOP, true>(a, ln, b, itX);
        f |= wm_sector<K, L, 1, STOP, true>(a, ln, b, itZ);
    } else {
        f = wm_sector<J, L, 0, STOP, false>(a, ln, b, itX);
        f |= wm_sector<K, L, 1, STOP, false>(a, ln, b, itZ);
    }
    wave_store_flags(a, ln, b, f, itX, itZ);
}

// ---- layered min-sum (QEC_OPT_MINSUM_SCHEDULE = 1; DESIGN.md section 2, "The layered min-sum form in the wave layout") ----
// The rule is sp_layered_decode's (bp_sparse.hip) in every bit.  The layers of a circulant-permutation code are its
// block rows, and a block row's checks sit one per lane, so a layer is one lane-local check pass.  The messages live in
// the VARIABLE view, Rv[r][l] = the message of row block r into the lane's variable of column l: the fold of a layer's
// inputs (the channel LLR and the R of the other row blocks, ascending) and the posterior are then lane-local adds,
// and a layer rotates its L inputs to the check view and its L outputs back -- per iteration the 2 (R - 1)(L - 1)
// permutes of a flooding iteration.  The stop tests and the flags read the posteriors; q_final is the posterior rotated
// to each check's slots, only when requested.  Frozen groups, full EXEC at every permute and the loop bound as above.
template <int R, int L>
__device__ __forceinline__ uint32_t wl_posterior(float (&post)[L], const float (&Rv)[R][L], const float (&lamv)[L], bool& in)
{
    uint32_t hd = 0;
    in = false;
#pragma unroll
    for (int l = 0; l < L; ++l) {
        float t = lamv[l];
#pragma unroll
        for (int r = 0; r < R; ++r) t = t + Rv[r][l];
        post[l] = t;
        hd |= (uint32_t)(t < 0.0f) << l;
        in |= wave_inside(t);
    }
    return hd;
}

template <int R, int L, int SEC, int STOP, bool FREEZE>
__device__ __forceinline__ uint32_t wl_sector(const WaveMinsumArgs& a, const WaveLane& ln, long long b, int& itn)
{
    const int P = a.P, n = a.n, N = a.maxIter;
    const int* D = SEC ? a.DZ : a.DX;
    const int* C = SEC ? a.CZ : a.CX;
    const float alpha = a.alpha;

    const uint32_t sb = wave_load_syndrome<R, SEC>(a, ln, b);
    // channel LLRs of the lane's variables (l, (i + C[l]) mod P)
    float lamv[L];
#pragma unroll
    for (int l = 0; l < L; ++l) lamv[l] = a.lam;
    if (a.llr != nullptr && ln.live) {
        const float* t = a.llr + (size_t)SEC * n;
#pragma unroll
        for (int l = 0; l < L; ++l) lamv[l] = t[l * P + wave_wrap(ln.i + C[l], P)];
    }
    float Rv[R][L];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int l = 0; l < L; ++l) Rv[r][l] = 0.0f;

    bool act = ln.live;  // the same on every lane of a group
    bool syn_ok = false; // syndrome stop: the last test of the group's own decisions
    itn = 0;
    for (int it = 0; it < N; ++it) {
        if (__builtin_amdgcn_ballot_w64(act) == 0ull) break;
        itn += act ? 1 : 0;
        {
            const WaveTable S = wave_table<WaveMinsumArgs, SEC>();
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float qc[L];
#pragma unroll
                for (int l = 0; l < L; ++l) {
                    float t = lamv[l];
#pragma unroll
                    for (int k = 0; k < R; ++k)
                        if (k != r) t = t + Rv[k][l];
                    qc[l] = (r == 0 || l == 0) ? t : wave_rot(t, ln, P - S[r * L + l]);
                }
                wave_check_row<L>(qc, ((sb >> (2 * r)) & 3u) != 0u, alpha);
#pragma unroll
                for (int l = 0; l < L; ++l) {
                    const float back = (r == 0 || l == 0) ? qc[l] : wave_rot(qc[l], ln, S[r * L + l]);
                    Rv[r][l] = FREEZE && !act ? Rv[r][l] : back;
                }
            }
        }
        if (STOP == QEC_STOP_REF && it % 10 == 0) {
            float post[L];
            bool in;
            (void)wl_posterior<R, L>(post, Rv, lamv, in);
            if (wave_group_all<true>(!in, ln)) act = false;
        } else if (STOP == QEC_STOP_SYNDROME) {
            float post[L];
            bool in;
            const uint32_t hd = wl_posterior<R, L>(post, Rv, lamv, in);
            const bool ok = wave_group_all<true>(wave_lane_syndrome_ok<R, L, SEC>(a, hd, sb, ln), ln);
            syn_ok = act ? ok : syn_ok;
            if (ok) act = false;
        }
    }

    // ---- the final state: posteriors, decisions, flags, the outputs ----
    float post[L];
    bool in;
    const uint32_t hd = wl_posterior<R, L>(post, Rv, lamv, in);
    const bool convFail = !wave_group_all<true>(!in, ln);
    if (STOP != QEC_STOP_SYNDROME || N == 0)
        syn_ok = wave_group_all<true>(wave_lane_syndrome_ok<R, L, SEC>(a, hd, sb, ln), ln);
    if (ln.live) {
        uint8_t* e = (SEC ? a.eZ : a.eX) + b * n;
#pragma unroll
        for (int l = 0; l < L; ++l) e[l * P + wave_wrap(ln.i + C[l], P)] = (uint8_t)((hd >> l) & 1u);
    }
    if (a.q != nullptr) {  // wave-uniform: every lane takes part in the rotations, a live lane stores
        const WaveTable S = wave_table<WaveMinsumArgs, SEC>();
        float* q = a.q + b * ((long long)(a.mX + a.mZ) * L) + (SEC ? (long long)a.mX * L : 0);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float* row = q + (size_t)(r * P + wave_wrap(ln.i + D[r], P)) * L;
#pragma unroll
            for (int l = 0; l < L; ++l) {
                const float v = (r == 0 || l == 0) ? post[l] : wave_rot(post[l], ln, P - S[r * L + l]);
                if (ln.live) row[l] = v;
            }
        }
    }
    uint32_t f = 0;
    if (!syn_ok) f |= SEC ? QEC_SYNDROME_FAIL_Z : QEC_SYNDROME_FAIL_X;
    if (convFail) f |= SEC ? QEC_CONVERGENCE_FAIL_Z : QEC_CONVERGENCE_FAIL_X;
    return f;
}

template <int J, int K, int L, int STOP>
__global__ __launch_bounds__(64) void wave_layered_kernel(const WaveMinsumArgs a)
{
    long long b;
    WaveLane ln;
    wave_lane(a, ln, b);

    uint32_t f;
    int itX, itZ;
    if (STOP != QEC_STOP_FIXED && a.G > 1) {  // wave-uniform: groups that stop on their own
        f = wl_sector<J, L, 0, STOP, true>(a, ln, b, itX);
        f |= wl_sector<K, L, 1, STOP, true>(a, ln, b, itZ);
    } else {
        f = wl_sector<J, L, 0, STOP, false>(a, ln, b, itX);
        f |= wl_sector<K, L, 1, STOP, false>(a, ln, b, itZ);
    }
    wave_store_flags(a, ln, b, f, itX, itZ);
}

// ---- the soft-syndrome form (qec_decoder_set_syndrome_priors) ----
// wm_sector and wl_sector with the virtual inputs, as bodies of their own: a shared body behind a template parameter
// changed the instruction streams of the kernels above.  mu = the sector's table, fo = its nullable output: every check
// has the virtual input mu_c; the lane keeps the decisions f of its R checks in fb, frozen with its group, and the
// syndrome tests XOR them into the parities.  The inside tests read the data slots / data posteriors as above.
template <int R, int L, int SEC, int STOP, bool FREEZE>
__device__ __forceinline__ uint32_t wm_sector_soft(const WaveMinsumArgs& a, const WaveLane& ln, long long b, int& itn,
                                                   const float* __restrict__ mu, uint8_t* __restrict__ fo)
{
    const int P = a.P, n = a.n, N = a.maxIter;
    const int* D = SEC ? a.DZ : a.DX;
    const int* C = SEC ? a.CZ : a.CX;
    const float alpha = a.alpha;

    const uint32_t sb = wave_load_syndrome<R, SEC>(a, ln, b);
    // channel LLRs of the lane's variables (l, (i + C[l]) mod P)
    float lamv[L];
#pragma unroll
    for (int l = 0; l < L; ++l) lamv[l] = a.lam;
    if (a.llr != nullptr && ln.live) {
        const float* t = a.llr + (size_t)SEC * n;
#pragma unroll
        for (int l = 0; l < L; ++l) lamv[l] = t[l * P + wave_wrap(ln.i + C[l], P)];
    }
    // every slot starts at its variable's channel LLR; the decisions of N = 0
    float m[R][L];
    uint32_t hd = 0;
    {
        const WaveTable S = wave_table<WaveMinsumArgs, SEC>();
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
                for (int r = 1; r < R; ++r) m[r][l] = wave_rot(lamv[l], ln, P - S[r * L + l]);
        }
    }

    float muv[R];
    uint32_t fb = 0;
    wave_load_mu<R, SEC>(muv, a, mu, ln);
#pragma unroll
    for (int r = 0; r < R; ++r) fb |= (uint32_t)(muv[r] < 0.0f) << r;  // N = 0
    auto lane_ok = [&]() { return wave_lane_syndrome_ok_soft<R, L, SEC>(a, hd, sb, fb, ln); };

    bool act = ln.live;  // the same on every lane of a group
    bool syn_ok = false; // syndrome stop: the last test of the group's own decisions
    itn = 0;
    for (int it = 0; it < N; ++it) {
        if (__builtin_amdgcn_ballot_w64(act) == 0ull) break;
        itn += act ? 1 : 0;
        fb = wave_check_pass_soft<R, L, FREEZE>(m, sb, muv, alpha, act, fb);
        if (it == N - 1) hd = wm_var_pass<R, L, SEC, true, FREEZE>(a, m, lamv, ln, act, hd);
        else hd = wm_var_pass<R, L, SEC, false, FREEZE>(a, m, lamv, ln, act, hd);
        if (STOP == QEC_STOP_REF && it % 10 == 0) {
            if (wave_group_all<true>(!wave_lane_any_inside<R, L>(m), ln)) act = false;
        } else if (STOP == QEC_STOP_SYNDROME) {
            const bool ok = wave_group_all<true>(lane_ok(), ln);
            syn_ok = act ? ok : syn_ok;
            if (ok) act = false;
        }
    }

    // ---- the final state: flags from the slots and from the decisions, the outputs ----
    const bool convFail = !wave_group_all<true>(!wave_lane_any_inside<R, L>(m), ln);
    if (STOP != QEC_STOP_SYNDROME || N == 0)
        syn_ok = wave_group_all<true>(lane_ok(), ln);
    if (fo != nullptr) wave_store_flips<R, SEC>(a, fo, ln, b, fb);  // wave-uniform
    if (ln.live) {
        uint8_t* e = (SEC ? a.eZ : a.eX) + b * n;
#pragma unroll
        for (int l = 0; l < L; ++l) e[l * P + wave_wrap(ln.i + C[l], P)] = (uint8_t)((hd >> l) & 1u);
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
    if (!syn_ok) f |= SEC ? QEC_SYNDROME_FAIL_Z : QEC_SYNDROME_FAIL_X;
    if (convFail) f |= SEC ? QEC_CONVERGENCE_FAIL_Z : QEC_CONVERGENCE_FAIL_X;
    return f;
}

template <int R, int L, int SEC, int STOP, bool FREEZE>
__device__ __forceinline__ uint32_t wl_sector_soft(const WaveMinsumArgs& a, const WaveLane& ln, long long b, int& itn,
                                                   const float* __restrict__ mu, uint8_t* __restrict__ fo)
{
    const int P = a.P, n = a.n, N = a.maxIter;
    const int* D = SEC ? a.DZ : a.DX;
    const int* C = SEC ? a.CZ : a.CX;
    const float alpha = a.alpha;

    const uint32_t sb = wave_load_syndrome<R, SEC>(a, ln, b);
    // channel LLRs of the lane's variables (l, (i + C[l]) mod P)
    float lamv[L];
#pragma unroll
    for (int l = 0; l < L; ++l) lamv[l] = a.lam;
    if (a.llr != nullptr && ln.live) {
        const float* t = a.llr + (size_t)SEC * n;
#pragma unroll
        for (int l = 0; l < L; ++l) lamv[l] = t[l * P + wave_wrap(ln.i + C[l], P)];
    }
    float Rv[R][L];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int l = 0; l < L; ++l) Rv[r][l] = 0.0f;
    float muv[R];
    uint32_t fb = 0;  // the decisions f of the lane's checks: R[c, virtual] = +0.0f at the start
    wave_load_mu<R, SEC>(muv, a, mu, ln);
#pragma unroll
    for (int r = 0; r < R; ++r) fb |= (uint32_t)(muv[r] < 0.0f) << r;
    auto lane_ok = [&](uint32_t hd) { return wave_lane_syndrome_ok_soft<R, L, SEC>(a, hd, sb, fb, ln); };

    bool act = ln.live;  // the same on every lane of a group
    bool syn_ok = false; // syndrome stop: the last test of the group's own decisions
    itn = 0;
    for (int it = 0; it < N; ++it) {
        if (__builtin_amdgcn_ballot_w64(act) == 0ull) break;
        itn += act ? 1 : 0;
        {
            const WaveTable S = wave_table<WaveMinsumArgs, SEC>();
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float qc[L];
#pragma unroll
                for (int l = 0; l < L; ++l) {
                    float t = lamv[l];
#pragma unroll
                    for (int k = 0; k < R; ++k)
                        if (k != r) t = t + Rv[k][l];
                    qc[l] = (r == 0 || l == 0) ? t : wave_rot(t, ln, P - S[r * L + l]);
                }
                const uint32_t f = (uint32_t)wave_check_row_soft<L>(qc, ((sb >> (2 * r)) & 3u) != 0u, muv[r], alpha) << r;
                fb = FREEZE && !act ? fb : ((fb & ~(1u << r)) | f);
#pragma unroll
                for (int l = 0; l < L; ++l) {
                    const float back = (r == 0 || l == 0) ? qc[l] : wave_rot(qc[l], ln, S[r * L + l]);
                    Rv[r][l] = FREEZE && !act ? Rv[r][l] : back;
                }
            }
        }
        if (STOP == QEC_STOP_REF && it % 10 == 0) {
            float post[L];
            bool in;
            (void)wl_posterior<R, L>(post, Rv, lamv, in);
            if (wave_group_all<true>(!in, ln)) act = false;
        } else if (STOP == QEC_STOP_SYNDROME) {
            float post[L];
            bool in;
            const uint32_t hd = wl_posterior<R, L>(post, Rv, lamv, in);
            const bool ok = wave_group_all<true>(lane_ok(hd), ln);
            syn_ok = act ? ok : syn_ok;
            if (ok) act = false;
        }
    }

    // ---- the final state: posteriors, decisions, flags, the outputs ----
    float post[L];
    bool in;
    const uint32_t hd = wl_posterior<R, L>(post, Rv, lamv, in);
    const bool convFail = !wave_group_all<true>(!in, ln);
    if (STOP != QEC_STOP_SYNDROME || N == 0)
        syn_ok = wave_group_all<true>(lane_ok(hd), ln);
    if (fo != nullptr) wave_store_flips<R, SEC>(a, fo, ln, b, fb);  // wave-uniform
    if (ln.live) {
        uint8_t* e = (SEC ? a.eZ : a.eX) + b * n;
#pragma unroll
        for (int l = 0; l < L; ++l) e[l * P + wave_wrap(ln.i + C[l], P)] = (uint8_t)((hd >> l) & 1u);
    }
    if (a.q != nullptr) {  // wave-uniform: every lane takes part in the rotations, a live lane stores
        const WaveTable S = wave_table<WaveMinsumArgs, SEC>();
        float* q = a.q + b * ((long long)(a.mX + a.mZ) * L) + (SEC ? (long long)a.mX * L : 0);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float* row = q + (size_t)(r * P + wave_wrap(ln.i + D[r], P)) * L;
#pragma unroll
            for (int l = 0; l < L; ++l) {
                const float v = (r == 0 || l == 0) ? post[l] : wave_rot(post[l], ln, P - S[r * L + l]);
                if (ln.live) row[l] = v;
            }
        }
    }
    uint32_t f = 0;
    if (!syn_ok) f |= SEC ? QEC_SYNDROME_FAIL_Z : QEC_SYNDROME_FAIL_X;
    if (convFail) f |= SEC ? QEC_CONVERGENCE_FAIL_Z : QEC_CONVERGENCE_FAIL_X;
    return f;
}

// The SOFT kernels: flooding and layered min-sum under syndrome priors, over the same shape table
template <int J, int K, int L, int STOP, bool LAYERED>
__global__ __launch_bounds__(64) void wave_soft_kernel(const WaveSoftArgs sa)
{
    const WaveMinsumArgs& a = sa.w;
    long long b;
    WaveLane ln;
    wave_lane(a, ln, b);

    const float* muX = sa.mu;
    const float* muZ = sa.mu + a.mX;
    uint32_t f;
    int itX, itZ;
    if (STOP != QEC_STOP_FIXED && a.G > 1) {  // wave-uniform: groups that stop on their own
        if constexpr (LAYERED) {
            f = wl_sector_soft<J, L, 0, STOP, true>(a, ln, b, itX, muX, sa.fX);
            f |= wl_sector_soft<K, L, 1, STOP, true>(a, ln, b, itZ, muZ, sa.fZ);
        } else {
            f = wm_sector_soft<J, L, 0, STOP, true>(a, ln, b, itX, muX, sa.fX);
            f |= wm_sector_soft<K, L, 1, STOP, true>(a, ln, b, itZ, muZ, sa.fZ);
        }
    } else {
        if constexpr (LAYERED) {
            f = wl_sector_soft<J, L, 0, STOP, false>(a, ln, b, itX, muX, sa.fX);
            f |= wl_sector_soft<K, L, 1, STOP, false>(a, ln, b, itZ, muZ, sa.fZ);
        } else {
            f = wm_sector_soft<J, L, 0, STOP, false>(a, ln, b, itX, muX, sa.fX);
            f |= wm_sector_soft<K, L, 1, STOP, false>(a, ln, b, itZ, muZ, sa.fZ);
        }
    }
    wave_store_flags(a, ln, b, f, itX, itZ);
}

// ---- host side ---------------------------------------------------------------
template <int J, int K, int L, bool LAYERED>
static WaveShape ws_shape_of()
{
    WaveShape s{J, K, L, {nullptr, nullptr, nullptr}};
    s.fn[QEC_STOP_REF] = reinterpret_cast<const void*>(&wave_soft_kernel<J, K, L, QEC_STOP_REF, LAYERED>);
    s.fn[QEC_STOP_FIXED] = reinterpret_cast<const void*>(&wave_soft_kernel<J, K, L, QEC_STOP_FIXED, LAYERED>);
    s.fn[QEC_STOP_SYNDROME] = reinterpret_cast<const void*>(&wave_soft_kernel<J, K, L, QEC_STOP_SYNDROME, LAYERED>);
    return s;
}
template <int J, int K, int L>
static WaveShape wsm_shape() { return ws_shape_of<J, K, L, false>(); }
template <int J, int K, int L>
static WaveShape wsl_shape() { return ws_shape_of<J, K, L, true>(); }

static const WaveShape kWaveSoftMinsumShapes[] = {QEC_WAVE_SHAPE_TABLE(wsm_shape)};
static const WaveShape kWaveSoftLayeredShapes[] = {QEC_WAVE_SHAPE_TABLE(wsl_shape)};

template <int J, int K, int L>
static WaveShape wl_shape()
{
    WaveShape s{J, K, L, {nullptr, nullptr, nullptr}};
    s.fn[QEC_STOP_REF] = reinterpret_cast<const void*>(&wave_layered_kernel<J, K, L, QEC_STOP_REF>);
    s.fn[QEC_STOP_FIXED] = reinterpret_cast<const void*>(&wave_layered_kernel<J, K, L, QEC_STOP_FIXED>);
    s.fn[QEC_STOP_SYNDROME] = reinterpret_cast<const void*>(&wave_layered_kernel<J, K, L, QEC_STOP_SYNDROME>);
    return s;
}

static const WaveShape kWaveLayeredShapes[] = {QEC_WAVE_SHAPE_TABLE(wl_shape)};

template <int J, int K, int L>
static WaveShape wm_shape()
{
    WaveShape s{J, K, L, {nullptr, nullptr, nullptr}};
    s.fn[QEC_STOP_REF] = reinterpret_cast<const void*>(&wave_minsum_kernel<J, K, L, QEC_STOP_REF>);
    s.fn[QEC_STOP_FIXED] = reinterpret_cast<const void*>(&wave_minsum_kernel<J, K, L, QEC_STOP_FIXED>);
    s.fn[QEC_STOP_SYNDROME] = reinterpret_cast<const void*>(&wave_minsum_kernel<J, K, L, QEC_STOP_SYNDROME>);
    return s;
}

static const WaveShape kWaveMinsumShapes[] = {QEC_WAVE_SHAPE_TABLE(wm_shape)};

// The wave min-sum kernels of a code, or nullptr (wave_find_shape).  No HIP call.
const void* select_wave_minsum(const Code& c) { return wave_find_shape(kWaveMinsumShapes, c); }

std::string wave_minsum_name(const Code& c) { return wave_name("minsum", c); }

// One min-sum decode launch in the wave layout: d as launch_decode_sparse's MINSUM kernels read it (minsum = the
// scale, lam, and with prior set llr), no relay tables; d.layered picks the layered kernels of the same shape.
int launch_wave_minsum(const void* shape, const Code& c, const SparseDecode& d, hipStream_t stream)
{
    const char* who = "wave min-sum launch";
    const WaveShape* s = static_cast<const WaveShape*>(shape);
    if (d.B <= 0) return QEC_OK;
    if (!wave_shape_fits(s, c)) return fail(QEC_ERR_ARG, "wave min-sum launch: the kernels are another code's");
    if (!d.minsum || d.corr || d.serial || d.gamma != nullptr)
        return fail(QEC_ERR_ARG, "wave min-sum launch: plain min-sum only (no correlated form, serial schedule or relay)");
    WaveMinsumArgs a{};
    const int rc = wave_fill_args(who, a, c, d);
    if (rc != QEC_OK) return rc;
    if (d.mu != nullptr) {  // syndrome priors: the SOFT kernels of the same shape
        s = d.layered ? wave_find_shape(kWaveSoftLayeredShapes, c) : wave_find_shape(kWaveSoftMinsumShapes, c);
        WaveSoftArgs sa{a, d.mu, d.fX, d.fZ};
        return wave_launch_as(who, s->fn[d.stop], sa, a.B, a.G, stream);
    }
    if (d.layered) s = wave_find_shape(kWaveLayeredShapes, c);  // the same row of the other table
    return wave_launch(who, s->fn[d.stop], a, stream);
}

}  // namespace qec
