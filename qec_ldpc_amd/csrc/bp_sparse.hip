// Sparse-graph BP engine: batched DecoderCPU::Decode (QEC_LDPC/DecoderCPU.h:150-390)
// for ANY code the reference's DecoderCPU accepts -- regular check degree dc = L and
// variable degree J (X) / K (Z), as its constructor assumes (DecoderCPU.h:296-311,
// InitIndexArrays :41-84) -- including codes that are not circulant-permutation QC
// codes, circulant codes with P > 64 and block shapes the wave-circulant engine
// (bp_decode.hip) has no instantiation for.
//
// Design: one workgroup per syndrome pair (grid-stride over the batch).  The X and Z
// Tanner graphs are decoded side by side in one message array, edge-major in the
// reference's own order (check c, slot k = its k-th variable in ascending id), which
// is also the q_final export layout:
//   msg[c * dc + k],  c in [0, mX) for X, [mX, mX + mZ) for Z.
// The array is LDS-resident when it fits (Etot * 4 B + syndrome/hard-decision bytes
// <= 160 KiB per workgroup on gfx950), otherwise it lives in a per-workgroup HBM
// scratch slice (L2-resident in practice).
//   * check pass: thread per check; reads its dc messages (contiguous), forms the
//     leave-one-out products in registers and overwrites them in place.
//   * variable pass: thread per variable; gathers its dv messages through the
//     varEdge table (edge ids in ascending check order), overwrites them in place.
// Each edge is owned by exactly one thread in each pass, so in-place updates are
// race-free; passes are separated by workgroup barriers.
//
// One kernel entry, bp_sparse_kernel<STOP, MAXDC, MAXDV, LDS, GENERAL, BODY>, under one argument block, SparseArgs (the
// SOFT and RELAY bodies append their own fields to it: SoftArgs, RelayArgs): it
// picks the workspace and calls the decode body that BODY names -- sp_flood_decode (the flooding schedule: kScalar with
// p', kPriors), sp_corr_decode (kCorr), sp_serial_decode (kSerial), sp_minsum_decode (kMinSum, kSoftMinSum),
// sp_relay_decode (kRelay: the min-sum body with a memory per variable and a chain of legs) and sp_layered_decode
// (kLayered, kSoftLayered).  Every body is templated on GENERAL -- false for a regular code, true for a code given by two
// matrices with any degrees -- which selects the table sentinels, the packed syndrome byte and the update functions;
// everything around the updates (loops, stop tests, post-processing, flags) is one text for both routes.  The plan keeps
// one table of kernels, by body and stop rule.
//
// Arithmetic is the same as the wave-circulant engine's (and so the reference's):
// left folds in ascending neighbour order (prefix reuse only), IEEE fp32 with
// denormals, -ffp-contract=off, correctly rounded division, and the two exact FMAs
// documented in bp_decode.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "../../include/HostDeviceArray.h"
#include "qec_internal.h"

#pragma clang fp contract(off)

namespace qec {

struct SparseArgs {
    const uint8_t* sX;
    const uint8_t* sZ;
    uint8_t* eX;
    uint8_t* eZ;
    uint8_t* flags;
    int32_t* iters;
    float* q;
    const int32_t* chkVar;   // (mX + mZ) x dc: sector-local variable ids, ascending
    const int32_t* varEdge;  // n x dvX (X) then n x dvZ (Z): edge ids, ascending check
    uint8_t* scratch;        // per-workgroup workspace in HBM (nullptr: LDS-resident)
    long long B;
    long long ws_bytes;      // workspace bytes per workgroup
    int n, mX, mZ, dc, dvX, dvZ;
    float errorProbability;
    int maxIter;
    const float* prior;      // PRIORS kernels: pi of sector X [n], then of sector Z [n] (qec_decoder_set_priors)
    // CORR kernels (QEC_OPT_CORRELATED): the first sector (0 = X, 1 = Z) and the second sector's conditional
    // priors -- with `prior` set the tables cond = c0_X [n], c1_X [n], c0_Z [n], c1_Z [n] (the first sector then
    // decodes under `prior`), without it the two scalars of qec_correlated_priors (the first sector under p')
    int first;
    float c0, c1;
    const float* cond;
    // SERIAL kernels (QEC_OPT_BP_SCHEDULE = 1): the processing order -- layOrder [mX + mZ], sector X's checks sorted
    // by (colour, index), then sector Z's (ids counted from mX) -- and the first position of each layer in it,
    // layOff = offX [LX + 1] (0 .. mX), then offZ [LZ + 1] (mX .. mX + mZ)
    const int32_t* layOrder;
    const int32_t* layOff;
    int LX, LZ;
    // a general code (dc = D, dvX / dvZ = the column strides): mX + mZ degree bytes; null for a regular code
    const uint8_t* chkDeg;
};

// The two bodies that need more than the block append their fields to it, at the offsets they always had: with the SOFT
// and RELAY fields in SparseArgs itself the SOFT kernels' instruction streams moved, and they measured up to 3.9 % slower
// on a small general code.
struct SoftArgs : SparseArgs {  // SOFT kernels (qec_decoder_set_syndrome_priors)
    const float* mu;         // mX + mZ channel LLRs of the measurement-error variables
    uint8_t* fX;             // nullable: [B][mX] measurement decisions out
    uint8_t* fZ;             // nullable: [B][mZ]
};

struct RelayArgs : SparseArgs {  // RELAY kernels (qec_decoder_set_relay)
    const float* gamma;      // [legs][sector][n]
    const int32_t* weight;   // null (w_v = 1), or sector X [n] then Z [n]: the handle's integer weight tables
    uint8_t* relayWs;        // per workgroup: M [2n] floats, best [2n] bytes
    long long relayStride;   // bytes per workgroup
    int legs, solutions;
};

static_assert(sizeof(SparseArgs) == 192 && sizeof(SoftArgs) == 216 && sizeof(RelayArgs) == 232,
              "the kernels' argument layouts: the block, then the body's own fields");

// The decode bodies, as the entry's BODY parameter and as the rows of the plan's kernel table.  kPriors is the flooding
// body's PRIORS form; CORR, SERIAL, MINSUM, RELAY and LAYERED take priors as a runtime branch.
enum { kScalar = 0, kPriors = 1, kCorr = 2, kSerial = 3, kMinSum = 4, kRelay = 5, kLayered = 6, kSoftMinSum = 7,
       kSoftLayered = 8, kVariants = 9 };

// The argument block of a body
template <int BODY> struct SparseArgsFor { using type = SparseArgs; };
template <> struct SparseArgsFor<kRelay> { using type = RelayArgs; };
template <> struct SparseArgsFor<kSoftMinSum> { using type = SoftArgs; };
template <> struct SparseArgsFor<kSoftLayered> { using type = SoftArgs; };
template <int BODY> using SparseArgsOf = typename SparseArgsFor<BODY>::type;

constexpr int kSparseThreads = 256;

__device__ __forceinline__ bool sp_inside(float x) { return x > 0.01f && x < 0.99f; }

// EqNodeUpdate (DecoderCPU.h:150-186) for one check: out_i = 0.5 -/+ 0.5 * prod_{k != i} (1 - 2 q_k)
template <int MAXDC>
__device__ __forceinline__ void sp_check(float* __restrict__ m, int dc, float h)
{
    float av[MAXDC];
#pragma unroll
    for (int k = 0; k < MAXDC; ++k)
        if (k < dc) av[k] = __builtin_fmaf(-2.0f, m[k], 1.0f);
    float pre = 1.0f;  // av[0] * ... * av[i-1], left fold from 1.0f (1.0f * x == x exactly)
#pragma unroll
    for (int i = 0; i < MAXDC; ++i) {
        if (i < dc) {
            float t = pre;
#pragma unroll
            for (int k = i + 1; k < MAXDC; ++k)
                if (k < dc) t = t * av[k];
            m[i] = __builtin_fmaf(h, t, 0.5f);  // safe in place: av[] already holds every input
            pre = pre * av[i];
        }
    }
}

// VarNodeUpdate (DecoderCPU.h:188-229) for one variable; returns its hard decision
// (any outgoing message >= 0.5f, DecoderCPU.h:354-373).
template <int MAXDV>
__device__ __forceinline__ bool sp_var(float* __restrict__ msg, const int32_t* __restrict__ ve, int dv, float pp,
                                       float omp, bool last)
{
    int idx[MAXDV];
    float g[MAXDV], bv[MAXDV], qv[MAXDV];
#pragma unroll
    for (int j = 0; j < MAXDV; ++j)
        if (j < dv) {
            idx[j] = ve[j];
            g[j] = msg[idx[j]];
            bv[j] = 1.0f - g[j];
        }
    if (last) {  // the final iteration includes the self message (DecoderCPU.h:216)
        float P0 = omp, P1 = pp;
#pragma unroll
        for (int k = 0; k < MAXDV; ++k)
            if (k < dv) { P0 = P0 * bv[k]; P1 = P1 * g[k]; }
        const float qq = P1 / (P0 + P1);
#pragma unroll
        for (int j = 0; j < MAXDV; ++j) qv[j] = qq;
    } else {
        float pre0 = omp, pre1 = pp;
#pragma unroll
        for (int j = 0; j < MAXDV; ++j)
            if (j < dv) {
                float t0 = pre0, t1 = pre1;
#pragma unroll
                for (int k = j + 1; k < MAXDV; ++k)
                    if (k < dv) { t0 = t0 * bv[k]; t1 = t1 * g[k]; }
                qv[j] = t1 / (t0 + t1);
                pre0 = pre0 * bv[j];
                pre1 = pre1 * g[j];
            }
    }
    bool hd = false;
#pragma unroll
    for (int j = 0; j < MAXDV; ++j)
        if (j < dv) {
            msg[idx[j]] = qv[j];
            hd |= qv[j] >= 0.5f;
        }
    return hd;
}

// ---- general codes (qec_code_from_matrices) -------------
// The same decode bodies (GENERAL) for a graph whose nodes have their own degrees.  Layout: msg[c * D + k] with
// one slot stride D (the largest row weight of both sectors); check c uses its first deg(c) slots and
// the others hold +0.0f from the initialisation to the q_final export.  Tables:
// chkVar [mX + mZ][D] and varEdge [n][dvX] / [n][dvZ] (the sectors' largest column weights), padded
// with -1, and one degree byte per check.
//   * check pass: a padded slot's input is +0.0f, so its factor fma(-2, 0, 1) is exactly 1.0f and
//     t * 1.0f == t bit for bit (denormals kept, a NaN stays that NaN): the folds run unpredicated over
//     the uniform stride D, behind the real factors, and only the store asks for the check's degree.
//     The degree travels in the check's LDS syndrome byte (bits 2..7; bits 0..1 = the entry as 0, 1 or
//     "other", all the update and the tests distinguish), so the pass reads nothing from global memory;
//     an unused slot is stored too, as +0.0f again (a select instead of a masked store).
//   * variable pass: the edge ids of the sector's stride are loaded unconditionally and the sentinel
//     tells which are real (they come first).  A padded entry enters the folds as g = 1 - g = 1.0f, the
//     same exact no-op, chosen by selects, so no arithmetic runs under a per-thread predicate: entry j is
//     skipped by a scalar branch when no thread of the wave has it (the compare's lane mask is that
//     test), computed by every lane otherwise, and only its store is masked -- and not even that when
//     every lane has it, which is every wave of a regular code.  A variable in no check touches nothing
//     and decides 0.
//   * the convergence test reads every slot: +0.0f is outside (0.01, 0.99), as a real hard message is.
//   * the syndrome tests and the final hard decision walk the whole stride and select on the sentinel
//     (an early exit would chain the table loads one behind the other).
// For a regular code D = L and every stored value equals the regular route's.
// The workgroup is the smallest of 64 / 128 / 256 threads that covers the wider pass, max(mX + mZ, 2n):
// a small code then pays for one or two waves at every barrier instead of four.
template <int MAXDC>
__device__ __forceinline__ void sp_check_general(float* __restrict__ m, int D, int deg, float h)
{
    float av[MAXDC];
#pragma unroll
    for (int k = 0; k < MAXDC; ++k)
        if (k < D) av[k] = __builtin_fmaf(-2.0f, m[k], 1.0f);
    float pre = 1.0f;
#pragma unroll
    for (int i = 0; i < MAXDC; ++i) {
        if (i < D) {
            float t = pre;
#pragma unroll
            for (int k = i + 1; k < MAXDC; ++k)
                if (k < D) t = t * av[k];
            m[i] = i < deg ? __builtin_fmaf(h, t, 0.5f) : 0.0f;  // an unused slot keeps +0.0f
            pre = pre * av[i];
        }
    }
}

template <int MAXDV>
__device__ __forceinline__ bool sp_var_general(float* __restrict__ msg, const int32_t* __restrict__ ve, int stride,
                                               float pp, float omp, bool last)
{
    int idx[MAXDV];
    bool any[MAXDV], all[MAXDV];  // wave-uniform: some / every active lane has entry j
    float g[MAXDV], bv[MAXDV], qv[MAXDV];
    const unsigned long long lanes = __builtin_amdgcn_ballot_w64(true);
#pragma unroll
    for (int j = 0; j < MAXDV; ++j) {
        idx[j] = -1;  // past the stride (which differs between the lanes of a wave that spans both sectors)
        if (j < stride) idx[j] = ve[j];
        const unsigned long long have = __builtin_amdgcn_ballot_w64(idx[j] >= 0);
        any[j] = have != 0;
        all[j] = have == lanes;
    }
#pragma unroll
    for (int j = 0; j < MAXDV; ++j)
        if (any[j]) {
            const bool real = idx[j] >= 0;
            // a padded lane reads slot 0, which its owner may be rewriting in this pass: the value is dropped
            // by the selects below, and any address inside the array serves
            const float x = msg[real ? idx[j] : 0];
            g[j] = real ? x : 1.0f;
            bv[j] = real ? 1.0f - x : 1.0f;
        }
    if (last) {
        float P0 = omp, P1 = pp;
#pragma unroll
        for (int k = 0; k < MAXDV; ++k)
            if (any[k]) { P0 = P0 * bv[k]; P1 = P1 * g[k]; }
        const float qq = P1 / (P0 + P1);
#pragma unroll
        for (int j = 0; j < MAXDV; ++j) qv[j] = qq;
    } else {
        float pre0 = omp, pre1 = pp;
#pragma unroll
        for (int j = 0; j < MAXDV; ++j)
            if (any[j]) {
                float t0 = pre0, t1 = pre1;
#pragma unroll
                for (int k = j + 1; k < MAXDV; ++k)
                    if (any[k]) { t0 = t0 * bv[k]; t1 = t1 * g[k]; }
                qv[j] = t1 / (t0 + t1);
                pre0 = pre0 * bv[j];
                pre1 = pre1 * g[j];
            }
    }
    bool hd = false;
#pragma unroll
    for (int j = 0; j < MAXDV; ++j)
        if (all[j]) {
            msg[idx[j]] = qv[j];
            hd |= qv[j] >= 0.5f;
        } else if (any[j]) {
            if (idx[j] >= 0) {
                msg[idx[j]] = qv[j];
                hd |= qv[j] >= 0.5f;
            }
        }
    return hd;
}

extern __shared__ __attribute__((aligned(16))) uint8_t sp_lds[];

// ---- pieces of the decode bodies ------------------------------------------------
// Every body is templated on GENERAL: false for a regular code's tables, true for a general code's padded
// ones.  sp_var_edges and sp_store_status serve every body; the others serve the flooding body and the min-sum
// family (MINSUM, RELAY, LAYERED), not CORR and SERIAL: calling them from those bodies, which spell the same
// steps out, changed those kernels' code and measured up to 2.6 % slower (profiles/flood_merge_ab.json).

// Syndromes in.  Regular: the entry as given -- the check update takes its truthiness, the syndrome tests compare
// it exactly (DecoderCPU.h:178, :381), so an entry other than 0/1 never matches a parity.  General: the entry as
// 0, 1 or 2 = any other value (truthy in the check update, never equal to a parity in the syndrome tests) with the
// check's degree above it.
template <bool GENERAL>
__device__ __forceinline__ void sp_load_syndromes(const SparseArgs& a, const uint8_t* chkDeg, long long b,
                                                  uint8_t* syn)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    const int mX = a.mX, mZ = a.mZ, m = mX + mZ;
    for (int c = tid; c < m; c += nt) {
        const uint32_t s = c < mX ? a.sX[b * mX + c] : a.sZ[b * mZ + (c - mX)];
        if (GENERAL) syn[c] = (uint8_t)((s > 1u ? 2u : s) | ((uint32_t)chkDeg[c] << 2));
        else syn[c] = (uint8_t)s;
    }
}

// One check's update in place, from its row of slots and its syndrome byte
template <int MAXDC, bool GENERAL>
__device__ __forceinline__ void sp_check_row(float* row, int dc, uint32_t sd)
{
    if (GENERAL) sp_check_general<MAXDC>(row, dc, (int)(sd >> 2), (sd & 3u) ? 0.5f : -0.5f);
    else sp_check<MAXDC>(row, dc, sd ? 0.5f : -0.5f);
}

// One variable's update; returns its hard decision
template <int MAXDV, bool GENERAL>
__device__ __forceinline__ bool sp_var_row(float* msg, const int32_t* ve, int dv, float pp,
                                           float omp, bool last)
{
    return GENERAL ? sp_var_general<MAXDV>(msg, ve, dv, pp, omp, last) : sp_var<MAXDV>(msg, ve, dv, pp, omp, last);
}

// One variable's row of the varEdge table and its stride; v runs over [X | Z], as the prior array does
__device__ __forceinline__ const int32_t* sp_var_edges(const SparseArgs& a, int v, int& dv)
{
    const bool z = v >= a.n;
    dv = z ? a.dvZ : a.dvX;
    return a.varEdge + (z ? (size_t)a.n * a.dvX + (size_t)(v - a.n) * dv : (size_t)v * dv);
}

// Whether the parity of one check (its chkVar row) over its sector's decision bytes h misses its syndrome byte.
// A general code walks the whole stride and selects on the sentinel: no early exit, the dc loads stay independent.
template <bool GENERAL>
__device__ __forceinline__ bool sp_parity_fails(const int32_t* row, int dc, const uint8_t* h, uint32_t sd)
{
    uint32_t x = 0;
    for (int k = 0; k < dc; ++k) {
        const int v = row[k];
        x ^= (!GENERAL || v >= 0) ? (uint32_t)h[v < 0 ? 0 : v] : 0u;
    }
    return x != (GENERAL ? (sd & 3u) : sd);
}

// The syndrome test over all checks of both sectors: bx / bz are set where a check fails
template <bool GENERAL>
__device__ __forceinline__ void sp_syndrome_fails(const SparseArgs& a, const uint8_t* syn, const uint8_t* hd, bool& bx,
                                                  bool& bz)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    const int mX = a.mX, m = mX + a.mZ, dc = a.dc;
    for (int c = tid; c < m; c += nt) {
        const bool z = c >= mX;
        if (sp_parity_fails<GENERAL>(a.chkVar + (size_t)c * dc, dc, hd + (z ? a.n : 0), syn[c])) {
            if (z) bz = true; else bx = true;
        }
    }
}

// The final hard decision of one variable: any message on its edges >= 0.5f (DecoderCPU.h:354-373)
template <bool GENERAL>
__device__ __forceinline__ bool sp_decide(const float* msg, const int32_t* ve, int dv)
{
    bool h = false;
    for (int j = 0; j < dv; ++j) {
        const int ed = ve[j];
        h |= (!GENERAL || ed >= 0) && msg[ed < 0 ? 0 : ed] >= 0.5f;
    }
    return h;
}

__device__ __forceinline__ uint32_t sp_fail_flags(bool synFailX, bool synFailZ, bool convFailX, bool convFailZ)
{
    uint32_t f = 0;
    if (synFailX) f |= QEC_SYNDROME_FAIL_X;
    if (synFailZ) f |= QEC_SYNDROME_FAIL_Z;
    if (convFailX) f |= QEC_CONVERGENCE_FAIL_X;
    if (convFailZ) f |= QEC_CONVERGENCE_FAIL_Z;
    return f;
}

// The flag word and the iteration counts of syndrome pair b, by thread 0
__device__ __forceinline__ void sp_store_status(const SparseArgs& a, long long b, uint32_t f, int itX, int itZ)
{
    if (threadIdx.x == 0) {
        a.flags[b] = (uint8_t)f;
        if (a.iters != nullptr) { a.iters[2 * b] = itX; a.iters[2 * b + 1] = itZ; }
    }
}

// ---- the flooding schedule: the scalar and the PRIORS kernels -------------------
// PRIORS: the per-variable prior form of DESIGN.md section 2 -- the initial message of a slot is the prior of
// its variable (through chkVar) and a variable's two running products start from 1 - pi_v and pi_v, read
// from global memory once per pass (8n bytes that every workgroup shares, so they stay in cache);
// errorProbability is unused.  Without it the body is the scalar one: PRIORS only selects operands.

// CheckConvergence (DecoderCPU.h:287-290) over every slot: whether a message of sector X / Z is inside (0.01, 0.99)
__device__ __forceinline__ void sp_any_inside(const float* msg, int E, int EX, bool& bx, bool& bz)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int e = tid; e < E; e += nt) {
        const bool in = sp_inside(msg[e]);
        if (e < EX) bx |= in; else bz |= in;
    }
}

template <int STOP, int MAXDC, int MAXDV, bool GENERAL, bool PRIORS>
__device__ __forceinline__ void sp_flood_decode(const SparseArgs& a, uint8_t* ws)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    const int n = a.n, mX = a.mX, mZ = a.mZ, m = mX + mZ, dc = a.dc;
    const int EX = mX * dc, E = m * dc;
    float* msg = reinterpret_cast<float*>(ws);            // E floats
    uint8_t* syn = ws + (size_t)E * sizeof(float);        // m bytes: sX then sZ
    uint8_t* hd = syn + m;                                // 2n bytes: X then Z hard decisions

    const float pp = 2.0f / 3.0f * a.errorProbability;   // DecoderCPU.h:259
    const float omp = 1.0f - pp;
    const int N = a.maxIter < 0 ? 0 : a.maxIter;

    for (long long b = blockIdx.x; b < a.B; b += gridDim.x) {
        sp_load_syndromes<GENERAL>(a, a.chkDeg, b, syn);
        // InitVarNodes: every edge starts at p' (DecoderCPU.h:135-148, 265-267) or at its variable's prior, one
        // edge per thread.  The check table is read only where it is needed: for the prior's index and for a
        // general code's sentinel, which tells a real slot from an unused one (coalesced words that every
        // workgroup reads, so they stay in cache).
        for (int e = tid; e < E; e += nt) {
            const int v = (GENERAL || PRIORS) ? a.chkVar[e] : 0;
            float x = 0.0f;  // an unused slot of a general code
            if (!GENERAL || v >= 0) x = PRIORS ? a.prior[(e < EX ? 0 : n) + v] : pp;
            msg[e] = x;
        }
        __syncthreads();

        bool actX = true, actZ = true;  // workgroup-uniform
        int itX = 0, itZ = 0;
        for (int it = 0; it < N && (actX || actZ); ++it) {  // BeliefPropogation, DecoderCPU.h:280-291
            const bool last = it == N - 1;
            itX += actX;
            itZ += actZ;
            for (int c = tid; c < m; c += nt) {
                if (c < mX ? !actX : !actZ) continue;
                sp_check_row<MAXDC, GENERAL>(msg + (size_t)c * dc, dc, syn[c]);
            }
            __syncthreads();
            for (int v = tid; v < 2 * n; v += nt) {
                if (v >= n ? !actZ : !actX) continue;
                int dv;
                const int32_t* ve = sp_var_edges(a, v, dv);
                const float pv = PRIORS ? a.prior[v] : pp;
                const bool h = sp_var_row<MAXDV, GENERAL>(msg, ve, dv, pv, PRIORS ? 1.0f - pv : omp, last);
                if (STOP == QEC_STOP_SYNDROME) hd[v] = h;
            }
            __syncthreads();
            if (STOP == QEC_STOP_REF && it % 10 == 0) {  // CheckConvergence, DecoderCPU.h:287-290
                bool bx = false, bz = false;
                sp_any_inside(msg, E, EX, bx, bz);
                const bool anyx = __syncthreads_or(bx), anyz = __syncthreads_or(bz);
                if (actX && !anyx) actX = false;
                if (actZ && !anyz) actZ = false;
            } else if (STOP == QEC_STOP_SYNDROME) {  // hard decision satisfies the syndrome
                bool bx = false, bz = false;
                sp_syndrome_fails<GENERAL>(a, syn, hd, bx, bz);
                const bool badx = __syncthreads_or(bx), badz = __syncthreads_or(bz);
                if (actX && !badx) actX = false;
                if (actZ && !badz) actZ = false;
            }
        }

        // ---- post-processing of Decode (DecoderCPU.h:354-384) ----
        bool bx = false, bz = false;
        sp_any_inside(msg, E, EX, bx, bz);
        for (int v = tid; v < 2 * n; v += nt) {
            int dv;
            const int32_t* ve = sp_var_edges(a, v, dv);
            const bool h = sp_decide<GENERAL>(msg, ve, dv);
            hd[v] = h;
            if (v >= n) a.eZ[b * n + (v - n)] = h; else a.eX[b * n + v] = h;
        }
        const bool convFailX = __syncthreads_or(bx), convFailZ = __syncthreads_or(bz);
        bool sx = false, sz = false;
        sp_syndrome_fails<GENERAL>(a, syn, hd, sx, sz);
        const bool synFailX = __syncthreads_or(sx), synFailZ = __syncthreads_or(sz);
        if (a.q != nullptr)
            for (int e = tid; e < E; e += nt) a.q[b * E + e] = msg[e];
        sp_store_status(a, b, sp_fail_flags(synFailX, synFailZ, convFailX, convFailZ), itX, itZ);
        __syncthreads();  // the workspace is reused by the next syndrome pair
    }
}

// ---- CORR: the correlated form (QEC_OPT_CORRELATED) -----
// The two sectors of a syndrome pair are decoded one after the other inside the workgroup, the first sector F
// (a.first) exactly as the flooding body decodes it -- the scalar p' or, with a.prior, its marginal priors -- and
// the second sector S by the prior form with pi_v = d[v] ? c1[v] : c0[v], d = F's final hard decisions, which
// stay in the workspace's hd bytes.  Workspace layout, grid and workgroup are the scalar plan's.  During a
// sector's passes the check pass runs threads [0, m_s) and the variable pass threads [0, n) of that sector
// only; each sector has its own iteration counter, last iteration and stop tests.  S's slots are initialised
// after F's post-processing, behind its barriers, through chkVar with the select on hd; a variable's thread
// reads its hd byte and its two table entries once per pass.  The updates are sp_check / sp_var (regular) or
// sp_check_general / sp_var_general (general: the exact no-op padding, unused slots +0.0f, a variable in no
// check decides 0), so every fp32 rule of the file carries over; one owner per edge per pass, no atomics.
template <int STOP, int MAXDC, int MAXDV, bool GENERAL>
__device__ __forceinline__ void sp_corr_decode(const SparseArgs& a, uint8_t* ws)
{
    const uint8_t* __restrict__ chkDeg = a.chkDeg;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int n = a.n, mX = a.mX, mZ = a.mZ, m = mX + mZ, dc = a.dc;
    const int E = m * dc;
    float* msg = reinterpret_cast<float*>(ws);            // E floats
    uint8_t* syn = ws + (size_t)E * sizeof(float);        // m bytes: sX then sZ
    uint8_t* hd = syn + m;                                // 2n bytes: X then Z hard decisions

    const float pp = 2.0f / 3.0f * a.errorProbability;
    const int N = a.maxIter < 0 ? 0 : a.maxIter;
    const bool tab = a.prior != nullptr;  // workgroup-uniform: tables (priors / a Pauli channel) or the scalar case

    for (long long b = blockIdx.x; b < a.B; b += gridDim.x) {
        for (int c = tid; c < m; c += nt) {
            const uint32_t s = c < mX ? a.sX[b * mX + c] : a.sZ[b * mZ + (c - mX)];
            if (GENERAL) syn[c] = (uint8_t)((s > 1u ? 2u : s) | ((uint32_t)chkDeg[c] << 2));
            else syn[c] = (uint8_t)s;
        }
        uint32_t f = 0;
        int itX = 0, itZ = 0;
        for (int pass = 0; pass < 2; ++pass) {
            const int sec = pass == 0 ? a.first : 1 - a.first;  // workgroup-uniform
            const bool second = pass == 1;
            const int c0 = sec ? mX : 0, ms = sec ? mZ : mX, dv = sec ? a.dvZ : a.dvX;
            const int e0 = c0 * dc, Es = ms * dc;
            const int32_t* veS = a.varEdge + (sec ? (size_t)n * a.dvX : 0);
            const float* pri = tab ? a.prior + (size_t)sec * n : nullptr;
            const float* t0 = tab ? a.cond + (size_t)sec * 2 * n : nullptr;
            const float* t1 = tab ? t0 + n : nullptr;
            uint8_t* hdS = hd + (size_t)sec * n;
            const uint8_t* hdF = hd + (size_t)(1 - sec) * n;  // read in the second pass only

            // the sector's slots: pi of the slot's variable (the second sector: selected by F's decision)
            for (int e = tid; e < Es; e += nt) {
                const int v = a.chkVar[e0 + e];
                float x = 0.0f;  // an unused slot of a general code
                if (!GENERAL || v >= 0) {
                    if (second) {
                        const bool d = hdF[v] != 0;
                        x = tab ? (d ? t1[v] : t0[v]) : (d ? a.c1 : a.c0);
                    } else {
                        x = tab ? pri[v] : pp;
                    }
                }
                msg[e0 + e] = x;
            }
            __syncthreads();

            bool act = true;  // workgroup-uniform
            int itn = 0;
            for (int it = 0; it < N && act; ++it) {
                const bool last = it == N - 1;
                ++itn;
                for (int c = tid; c < ms; c += nt) {
                    const uint32_t sd = syn[c0 + c];
                    if (GENERAL)
                        sp_check_general<MAXDC>(msg + (size_t)(c0 + c) * dc, dc, (int)(sd >> 2), (sd & 3u) ? 0.5f : -0.5f);
                    else
                        sp_check<MAXDC>(msg + (size_t)(c0 + c) * dc, dc, sd ? 0.5f : -0.5f);
                }
                __syncthreads();
                for (int v = tid; v < n; v += nt) {
                    float pv;
                    if (second) {
                        const bool d = hdF[v] != 0;
                        pv = tab ? (d ? t1[v] : t0[v]) : (d ? a.c1 : a.c0);
                    } else {
                        pv = tab ? pri[v] : pp;
                    }
                    const int32_t* ve = veS + (size_t)v * dv;
                    const bool h = GENERAL ? sp_var_general<MAXDV>(msg, ve, dv, pv, 1.0f - pv, last)
                                           : sp_var<MAXDV>(msg, ve, dv, pv, 1.0f - pv, last);
                    if (STOP == QEC_STOP_SYNDROME) hdS[v] = h;
                }
                __syncthreads();
                if (STOP == QEC_STOP_REF && it % 10 == 0) {
                    bool in = false;
                    for (int e = tid; e < Es; e += nt) in |= sp_inside(msg[e0 + e]);
                    act = __syncthreads_or(in);
                } else if (STOP == QEC_STOP_SYNDROME) {
                    bool bad = false;
                    for (int c = tid; c < ms; c += nt) {
                        uint32_t x = 0;
                        for (int k = 0; k < dc; ++k) {
                            const int v = a.chkVar[(size_t)(c0 + c) * dc + k];
                            x ^= (!GENERAL || v >= 0) ? (uint32_t)hdS[v < 0 ? 0 : v] : 0u;
                        }
                        bad |= x != (GENERAL ? (syn[c0 + c] & 3u) : (uint32_t)syn[c0 + c]);
                    }
                    act = __syncthreads_or(bad);
                }
            }

            // ---- post-processing of Decode for this sector ----
            bool in = false;
            for (int e = tid; e < Es; e += nt) in |= sp_inside(msg[e0 + e]);
            uint8_t* eOut = sec ? a.eZ : a.eX;
            for (int v = tid; v < n; v += nt) {
                const int32_t* ve = veS + (size_t)v * dv;
                bool h = false;
                for (int j = 0; j < dv; ++j) {
                    const int ed = ve[j];
                    h |= (!GENERAL || ed >= 0) && msg[ed < 0 ? 0 : ed] >= 0.5f;
                }
                hdS[v] = h;
                eOut[b * n + v] = h;
            }
            const bool convFail = __syncthreads_or(in);
            bool bad = false;
            for (int c = tid; c < ms; c += nt) {
                uint32_t x = 0;
                for (int k = 0; k < dc; ++k) {
                    const int v = a.chkVar[(size_t)(c0 + c) * dc + k];
                    x ^= (!GENERAL || v >= 0) ? (uint32_t)hdS[v < 0 ? 0 : v] : 0u;
                }
                bad |= x != (GENERAL ? (syn[c0 + c] & 3u) : (uint32_t)syn[c0 + c]);
            }
            const bool synFail = __syncthreads_or(bad);
            if (synFail) f |= sec ? QEC_SYNDROME_FAIL_Z : QEC_SYNDROME_FAIL_X;
            if (convFail) f |= sec ? QEC_CONVERGENCE_FAIL_Z : QEC_CONVERGENCE_FAIL_X;
            if (sec) itZ = itn; else itX = itn;
        }
        if (a.q != nullptr)
            for (int e = tid; e < E; e += nt) a.q[b * E + e] = msg[e];
        sp_store_status(a, b, f, itX, itZ);
        __syncthreads();  // the workspace is reused by the next syndrome pair
    }
}

// ---- SERIAL: the serial schedule (QEC_OPT_BP_SCHEDULE = 1) -----
// The message array holds R, the check->variable message of every edge: 0.5f at the start, an unused slot of a
// general code +0.0f throughout.  An iteration walks the layers; a layer interval takes the X checks of colour l and,
// behind them, the Z checks of colour l, in two steps with a barrier behind each (striding over the workgroup when a
// layer is larger):
//   * a thread per slot of those checks forms the message of the slot's variable from the R of the variable's other
//     checks -- a plain ascending loop over its varEdge row with two scalar accumulators, its own edge told by the
//     edge id -- and parks it in its own slot, which nobody else reads in this interval: the checks of one colour
//     share no variable, so an edge of these checks is read only for checks of other colours, in other intervals;
//   * a thread per check turns its row into the check's R in place by sp_check / sp_check_general, as in the
//     flooding kernels.
// Each R[e] is thus written by one thread per step and read by threads of other intervals: no atomics.  A sector
// with fewer layers idles in the remaining intervals, a stopped sector in all of them.  (The one-step form, a thread
// per check forming its own slots one after the other, keeps 6 of hgp_ham's 128 threads busy and measured 1.4 to 2.9
// times slower per iteration: profiles/serial_edge_ab.json.)
// The posterior pass (thread per variable, the same loop over all of the variable's checks) writes the decision bytes
// and folds the inside test into its ballot; it runs where a stop rule looks (syndrome stop: every iteration,
// reference stop: iterations with index % 10 == 0) and once on the final state.  The q_final export recomputes the
// posterior per edge, only when q is requested.  Workspace, grid and workgroup are the scalar plan's.
template <bool GENERAL>
__device__ __forceinline__ float sp_serial_fold(const float* __restrict__ msg, const int32_t* __restrict__ ve, int dv,
                                                int self, float pv)
{
    float P0 = 1.0f - pv, P1 = pv;
    for (int j = 0; j < dv; ++j) {
        const int ed = ve[j];
        if (GENERAL && ed < 0) break;  // the real entries come first
        if (ed == self) continue;
        const float r = msg[ed];
        P0 = P0 * (1.0f - r);
        P1 = P1 * r;
    }
    return P1 / (P0 + P1);
}

template <int STOP, int MAXDC, int MAXDV, bool GENERAL>
__device__ __forceinline__ void sp_serial_decode(const SparseArgs& a, uint8_t* ws)
{
    const uint8_t* __restrict__ chkDeg = a.chkDeg;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int n = a.n, mX = a.mX, mZ = a.mZ, m = mX + mZ, dc = a.dc;
    const int EX = mX * dc, E = m * dc;
    float* msg = reinterpret_cast<float*>(ws);            // E floats
    uint8_t* syn = ws + (size_t)E * sizeof(float);        // m bytes: sX then sZ
    uint8_t* hd = syn + m;                                // 2n bytes: X then Z hard decisions

    const float pp = 2.0f / 3.0f * a.errorProbability;
    const int N = a.maxIter < 0 ? 0 : a.maxIter;
    const bool tab = a.prior != nullptr;  // workgroup-uniform: per-variable priors or the scalar p'
    const int LX = a.LX, LZ = a.LZ;
    const int32_t* offX = a.layOff;
    const int32_t* offZ = a.layOff + LX + 1;

    // the posterior pass over the sectors doX / doZ: decision bytes, and whether a posterior is inside (0.01, 0.99)
    auto posterior = [&](bool doX, bool doZ, bool& bx, bool& bz) {
        for (int v = tid; v < 2 * n; v += nt) {
            const bool z = v >= n;
            if (z ? !doZ : !doX) continue;
            int dv;
            const int32_t* ve = sp_var_edges(a, v, dv);
            if (GENERAL && ve[0] < 0) { hd[v] = 0; continue; }  // a variable in no check decides 0, enters no test
            const float post = sp_serial_fold<GENERAL>(msg, ve, dv, -1, tab ? a.prior[v] : pp);
            hd[v] = post >= 0.5f;
            if (sp_inside(post)) { if (z) bz = true; else bx = true; }
        }
    };
    auto syndrome_bad = [&](bool& bx, bool& bz) {
        for (int c = tid; c < m; c += nt) {
            const bool z = c >= mX;
            const uint8_t* h = hd + (z ? n : 0);
            uint32_t x = 0;
            for (int k = 0; k < dc; ++k) {
                const int v = a.chkVar[(size_t)c * dc + k];
                x ^= (!GENERAL || v >= 0) ? (uint32_t)h[v < 0 ? 0 : v] : 0u;
            }
            if (x != (GENERAL ? (syn[c] & 3u) : (uint32_t)syn[c])) { if (z) bz = true; else bx = true; }
        }
    };

    for (long long b = blockIdx.x; b < a.B; b += gridDim.x) {
        for (int c = tid; c < m; c += nt) {
            const uint32_t s = c < mX ? a.sX[b * mX + c] : a.sZ[b * mZ + (c - mX)];
            if (GENERAL) syn[c] = (uint8_t)((s > 1u ? 2u : s) | ((uint32_t)chkDeg[c] << 2));
            else syn[c] = (uint8_t)s;
        }
        for (int e = tid; e < E; e += nt) msg[e] = (!GENERAL || a.chkVar[e] >= 0) ? 0.5f : 0.0f;
        __syncthreads();

        bool actX = true, actZ = true;  // workgroup-uniform
        int itX = 0, itZ = 0;
        for (int it = 0; it < N && (actX || actZ); ++it) {
            itX += actX;
            itZ += actZ;
            const int layers = max(actX ? LX : 0, actZ ? LZ : 0);
            for (int l = 0; l < layers; ++l) {
                const int x0 = actX && l < LX ? offX[l] : 0, nx = actX && l < LX ? offX[l + 1] - x0 : 0;
                const int z0 = actZ && l < LZ ? offZ[l] : 0, nz = actZ && l < LZ ? offZ[l + 1] - z0 : 0;
                // the slots of the layer's checks, a thread per slot: the message of the slot's variable
                for (int i = tid; i < (nx + nz) * dc; i += nt) {
                    const int j = i / dc, k = i - j * dc;
                    const int c = a.layOrder[j < nx ? x0 + j : z0 + (j - nx)];
                    const int e = c * dc + k, v = a.chkVar[e];
                    if (GENERAL && v < 0) continue;  // an unused slot keeps +0.0f
                    const bool z = c >= mX;
                    const int dv = z ? a.dvZ : a.dvX;
                    const int32_t* ve = a.varEdge + (z ? (size_t)n * a.dvX : 0) + (size_t)v * dv;
                    msg[e] = sp_serial_fold<GENERAL>(msg, ve, dv, e, tab ? a.prior[(z ? n : 0) + v] : pp);
                }
                __syncthreads();
                // the layer's checks, a thread per check: the row becomes the check's R
                for (int i = tid; i < nx + nz; i += nt) {
                    const int c = a.layOrder[i < nx ? x0 + i : z0 + (i - nx)];
                    const uint32_t sd = syn[c];
                    if (GENERAL) sp_check_general<MAXDC>(msg + (size_t)c * dc, dc, (int)(sd >> 2), (sd & 3u) ? 0.5f : -0.5f);
                    else sp_check<MAXDC>(msg + (size_t)c * dc, dc, sd ? 0.5f : -0.5f);
                }
                __syncthreads();
            }
            if (STOP == QEC_STOP_REF && it % 10 == 0) {
                bool bx = false, bz = false;
                posterior(actX, actZ, bx, bz);
                const bool anyx = __syncthreads_or(bx), anyz = __syncthreads_or(bz);
                if (actX && !anyx) actX = false;
                if (actZ && !anyz) actZ = false;
            } else if (STOP == QEC_STOP_SYNDROME) {
                bool bx = false, bz = false;
                posterior(actX, actZ, bx, bz);
                __syncthreads();
                bx = bz = false;
                syndrome_bad(bx, bz);
                const bool badx = __syncthreads_or(bx), badz = __syncthreads_or(bz);
                if (actX && !badx) actX = false;
                if (actZ && !badz) actZ = false;
            }
        }

        // ---- the final state: decisions, flags, q_final ----
        bool bx = false, bz = false;
        posterior(true, true, bx, bz);
        const bool convFailX = __syncthreads_or(bx), convFailZ = __syncthreads_or(bz);
        for (int v = tid; v < 2 * n; v += nt) {
            if (v >= n) a.eZ[b * n + (v - n)] = hd[v]; else a.eX[b * n + v] = hd[v];
        }
        bool sx = false, sz = false;
        syndrome_bad(sx, sz);
        const bool synFailX = __syncthreads_or(sx), synFailZ = __syncthreads_or(sz);
        if (a.q != nullptr)
            for (int e = tid; e < E; e += nt) {
                const int v = a.chkVar[e];
                float post = 0.0f;  // an unused slot of a general code
                if (!GENERAL || v >= 0) {
                    const int gv = (e < EX ? 0 : n) + v;
                    int dv;
                    const int32_t* ve = sp_var_edges(a, gv, dv);
                    post = sp_serial_fold<GENERAL>(msg, ve, dv, -1, tab ? a.prior[gv] : pp);
                }
                a.q[b * E + e] = post;
            }
        sp_store_status(a, b, sp_fail_flags(synFailX, synFailZ, convFailX, convFailZ), itX, itZ);
        __syncthreads();  // the workspace is reused by the next syndrome pair
    }
}

// ---- MINSUM: scaled min-sum in the LLR domain (QEC_OPT_BP_METHOD = 1) -----
// The flooding schedule over LLRs (> 0: the bit is 0): the message array holds the variable->check message of every
// edge after a variable pass and the check->variable message after a check pass, as in the flooding body, with the
// barriers where that body has them.  Only fp32 adds, one fp32 multiply by alpha = k / 256 and integer operations on
// bit patterns occur, so every value is finite.  The min-sum family reads three fields of the argument block its own
// way: errorProbability carries the scalar channel LLR lambda(p'), prior (workgroup-uniform: null or not) the 2n
// channel LLRs of the handle's priors, c0 the factor alpha.
//   * check pass: thread per check, one pass over its row for the first minimum, the second minimum and the argmin
//     of the magnitudes' bit patterns (compared as unsigned integers, capped by K = the pattern of 2^20) and the XOR
//     of the sign bits with the syndrome bit; a second pass stores alpha * (second minimum where the slot is the
//     argmin, else the first) under the slot's sign.  Five live values instead of the product rule's MAXDC factors;
//     the row is read twice from the workspace instead.  (Keeping the row's MAXDC patterns in registers between the
//     passes, loaded together as sp_check loads them, measured 8 % faster per iteration on hgp_ham and 6 % / 9 %
//     slower on QC_LDPC_CSS(3,3,6,13,3,2) / P61: profiles/minsum.json, cost_row_in_registers.)
//   * a general code's unused slot holds the float K throughout: sign 0 and a magnitude that is not below the cap,
//     so it changes neither a minimum nor the parity; it is stored back as K by a select on the check's degree, is
//     outside the inside band by itself, and the export writes +0.0f for it.
//   * variable pass: thread per variable, the prefix form of sp_var with + for * and no division.  A general code's
//     padded entry enters the folds as +0.0f, chosen by a select, behind the real ones.  x + (+0.0f) == x bit for
//     bit for every finite x but -0.0f, and a fold never holds -0.0f there: it starts from a channel LLR, which
//     minsum_llr never returns as -0.0f, and a sum of two floats is -0.0f only when both are.  So the padding is
//     exact without a predicate on the adds; entry j is skipped by a scalar branch when no lane of the wave has it.
//     The fold over all entries is the posterior; its sign is the decision byte, written every iteration.
//   * the post-processing reads the decision bytes of the last executed variable pass (N = 0: of the channel LLRs).
__device__ __forceinline__ bool sp_minsum_inside(float x) { return __builtin_fabsf(x) < kMinSumInside; }

template <bool GENERAL>
__device__ __forceinline__ void sp_minsum_check(float* __restrict__ m, int dc, uint32_t sd, float alpha)
{
    uint32_t min1 = kMinSumCap, min2 = kMinSumCap;
    uint32_t par = GENERAL ? ((sd & 3u) != 0u) : (sd != 0u);
    int arg = -1;
    for (int k = 0; k < dc; ++k) {
        const uint32_t b = __float_as_uint(m[k]);
        const uint32_t a = b & 0x7FFFFFFFu;
        par ^= b >> 31;
        const bool lt1 = a < min1, lt2 = a < min2;
        min2 = lt1 ? min1 : lt2 ? a : min2;
        arg = lt1 ? k : arg;
        min1 = lt1 ? a : min1;
    }
    const uint32_t o1 = __float_as_uint(alpha * __uint_as_float(min1));
    const uint32_t o2 = __float_as_uint(alpha * __uint_as_float(min2));
    const int deg = GENERAL ? (int)(sd >> 2) : dc;
    for (int i = 0; i < dc; ++i) {
        const uint32_t b = __float_as_uint(m[i]);
        const uint32_t o = (i == arg ? o2 : o1) | ((par ^ (b >> 31)) << 31);
        m[i] = __uint_as_float(!GENERAL || i < deg ? o : kMinSumCap);  // an unused slot keeps K
    }
}

// SOFT: min-sum under syndrome priors (qec_decoder_set_syndrome_priors; DESIGN.md section 2, "The soft-syndrome form").
// The SOFT instantiations of the MINSUM and LAYERED bodies; the others do not change.  Check c has one virtual input mu[c],
// the channel LLR of its measurement-error variable, read from the handle's table (mX + mZ floats that every workgroup
// shares).  The syndrome byte of the workspace holds the entry as 0, 1 or 2 = any other value in bits 0-1 and the measurement
// decision f_c in bit 2 (a general code's degree is read from chkDeg instead): the thread that updates check c rewrites the
// byte, the syndrome tests XOR the bit into the row's parity.  No further workspace.  The SOFT bodies keep helpers of their
// own (sp_soft_load_syndromes, sp_soft_check, sp_soft_syndrome_fails) and their pointers as __restrict__ parameters: folded
// into the plain helpers' SOFT forms, or read from the block, their kernels' instruction streams moved and a small general
// code measured up to 3.9 % slower.
__device__ __forceinline__ void sp_soft_load_syndromes(const SparseArgs& a, const float* __restrict__ mu, long long b,
                                                       uint8_t* syn)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    const int mX = a.mX, mZ = a.mZ, m = mX + mZ;
    for (int c = tid; c < m; c += nt) {
        const uint32_t s = c < mX ? a.sX[b * mX + c] : a.sZ[b * mZ + (c - mX)];
        syn[c] = (uint8_t)((s > 1u ? 2u : s) | (mu[c] < 0.0f ? 4u : 0u));  // f of N = 0 (layered: of R = +0.0f)
    }
}

// sp_minsum_check with the virtual input: it enters the minima and the sign XOR ahead of the row (the outputs do not
// depend on an input's position); returns f = mu + rho < 0, rho the virtual slot's own output
template <bool GENERAL>
__device__ __forceinline__ bool sp_soft_check(float* __restrict__ m, int dc, int deg, uint32_t sd, float mu, float alpha)
{
    const uint32_t mb = __float_as_uint(mu), ma = mb & 0x7FFFFFFFu;
    const bool virt = ma < kMinSumCap;
    uint32_t min1 = virt ? ma : kMinSumCap, min2 = kMinSumCap;
    uint32_t par = ((sd & 3u) != 0u) ^ (mb >> 31);
    int arg = virt ? -2 : -1;
    for (int k = 0; k < dc; ++k) {
        const uint32_t b = __float_as_uint(m[k]);
        const uint32_t a = b & 0x7FFFFFFFu;
        par ^= b >> 31;
        const bool lt1 = a < min1, lt2 = a < min2;
        min2 = lt1 ? min1 : lt2 ? a : min2;
        arg = lt1 ? k : arg;
        min1 = lt1 ? a : min1;
    }
    const uint32_t o1 = __float_as_uint(alpha * __uint_as_float(min1));
    const uint32_t o2 = __float_as_uint(alpha * __uint_as_float(min2));
    for (int i = 0; i < dc; ++i) {
        const uint32_t b = __float_as_uint(m[i]);
        const uint32_t o = (i == arg ? o2 : o1) | ((par ^ (b >> 31)) << 31);
        m[i] = __uint_as_float(!GENERAL || i < deg ? o : kMinSumCap);  // an unused slot keeps K
    }
    const float rho = __uint_as_float((arg == -2 ? o2 : o1) | ((par ^ (mb >> 31)) << 31));
    const float postm = mu + rho;
    return postm < 0.0f;
}

// sp_syndrome_fails under SOFT: check c is satisfied iff (the row's parity) ^ f_c equals its syndrome entry exactly
template <bool GENERAL>
__device__ __forceinline__ void sp_soft_syndrome_fails(const SparseArgs& a, const uint8_t* syn, const uint8_t* hd, bool& bx,
                                                       bool& bz)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    const int mX = a.mX, m = mX + a.mZ, dc = a.dc;
    for (int c = tid; c < m; c += nt) {
        const bool z = c >= mX;
        const int32_t* row = a.chkVar + (size_t)c * dc;
        const uint8_t* h = hd + (z ? a.n : 0);
        const uint32_t sd = syn[c];
        uint32_t x = (sd >> 2) & 1u;
        for (int k = 0; k < dc; ++k) {
            const int v = row[k];
            x ^= (!GENERAL || v >= 0) ? (uint32_t)h[v < 0 ? 0 : v] : 0u;
        }
        if (x != (sd & 3u)) {
            if (z) bz = true; else bx = true;
        }
    }
}

// Check c's update in place, from its row of slots and its syndrome byte; SOFT rewrites the byte with the new f_c.
// dc is the caller's copy of the block's dc.
template <bool GENERAL, bool SOFT>
__device__ __forceinline__ void sp_minsum_check_row(const uint8_t* chkDeg, const float* mu, float* msg, uint8_t* syn, int c,
                                                    int dc, float alpha)
{
    if constexpr (SOFT) {
        const uint32_t sd = syn[c];
        const bool f = sp_soft_check<GENERAL>(msg + (size_t)c * dc, dc, GENERAL ? (int)chkDeg[c] : dc, sd, mu[c], alpha);
        syn[c] = (uint8_t)((sd & 3u) | (f ? 4u : 0u));
    } else {
        sp_minsum_check<GENERAL>(msg + (size_t)c * dc, dc, syn[c], alpha);
    }
}

// The measurement decisions of syndrome pair b out, where requested
__device__ __forceinline__ void sp_soft_store_flips(const SparseArgs& a, long long b, const uint8_t* syn, uint8_t* fX, uint8_t* fZ)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    const int mX = a.mX, mZ = a.mZ;
    if (fX != nullptr)
        for (int c = tid; c < mX; c += nt) fX[b * mX + c] = (syn[c] >> 2) & 1u;
    if (fZ != nullptr)
        for (int c = tid; c < mZ; c += nt) fZ[b * mZ + c] = (syn[mX + c] >> 2) & 1u;
}

// One variable's update, the folds started from the bias `lam` (MINSUM: its channel LLR, RELAY: the leg's mix of that and
// the memory, never -0.0f); returns the posterior and decides through `dec` (posterior < 0; a variable in no check
// decides 0)
template <int MAXDV, bool GENERAL>
__device__ __forceinline__ float sp_minsum_var(float* __restrict__ msg, const int32_t* __restrict__ ve, int dv, float lam,
                                               bool last, bool& dec)
{
    int idx[MAXDV];
    bool use[MAXDV];  // GENERAL: wave-uniform, some active lane has entry j
    float r[MAXDV];
#pragma unroll
    for (int j = 0; j < MAXDV; ++j) {
        idx[j] = -1;  // past the stride (which differs between the lanes of a wave that spans both sectors)
        if (j < dv) idx[j] = ve[j];
        use[j] = GENERAL ? __builtin_amdgcn_ballot_w64(idx[j] >= 0) != 0 : j < dv;
    }
#pragma unroll
    for (int j = 0; j < MAXDV; ++j)
        if (use[j]) {
            const bool real = idx[j] >= 0;
            // a padded lane reads slot 0, which its owner may be rewriting in this pass: the select drops the value
            const float x = msg[real ? idx[j] : 0];
            r[j] = real ? x : 0.0f;
        }
    float post = lam;
    if (last) {  // the last iteration of the cap: every slot receives the posterior
#pragma unroll
        for (int k = 0; k < MAXDV; ++k)
            if (use[k]) post = post + r[k];
#pragma unroll
        for (int j = 0; j < MAXDV; ++j)
            if (use[j] && idx[j] >= 0) msg[idx[j]] = post;
    } else {
        // in place: every incoming message is in r[] already, and the edge has no other owner in this pass
#pragma unroll
        for (int j = 0; j < MAXDV; ++j)
            if (use[j]) {
                float t = post;  // lam + r_0 + ... + r_{j-1}
#pragma unroll
                for (int k = j + 1; k < MAXDV; ++k)
                    if (use[k]) t = t + r[k];
                if (idx[j] >= 0) msg[idx[j]] = t;
                post = post + r[j];
            }
    }
    dec = idx[0] >= 0 && post < 0.0f;
    return post;
}

template <int STOP, int MAXDC, int MAXDV, bool GENERAL, bool SOFT>
__device__ __forceinline__ void sp_minsum_decode(const SparseArgs& a, const uint8_t* __restrict__ chkDeg, uint8_t* ws,
        const float* __restrict__ mu = nullptr, uint8_t* fX = nullptr, uint8_t* fZ = nullptr)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    const int n = a.n, mX = a.mX, mZ = a.mZ, m = mX + mZ, dc = a.dc;
    const int EX = mX * dc, E = m * dc;
    float* msg = reinterpret_cast<float*>(ws);            // E floats
    uint8_t* syn = ws + (size_t)E * sizeof(float);        // m bytes: sX then sZ
    uint8_t* hd = syn + m;                                // 2n bytes: X then Z decisions

    const float lam0 = a.errorProbability, alpha = a.c0;
    const float* llr = a.prior;
    const bool tab = llr != nullptr;  // workgroup-uniform: per-variable channel LLRs or the scalar one
    const int N = a.maxIter < 0 ? 0 : a.maxIter;

    // The inside test, the slot initialisation and the q_final export are spelled out here and again in sp_relay_decode:
    // as shared helpers each of them moved the instruction streams of RELAY or MINSUM kernels that are otherwise the
    // parent's ("tried, changed the streams").
    auto any_inside = [&](bool& bx, bool& bz) {
        for (int e = tid; e < E; e += nt) {
            const bool in = sp_minsum_inside(msg[e]);
            if (e < EX) bx |= in; else bz |= in;
        }
    };

    for (long long b = blockIdx.x; b < a.B; b += gridDim.x) {
        if constexpr (SOFT) sp_soft_load_syndromes(a, mu, b, syn); else sp_load_syndromes<GENERAL>(a, chkDeg, b, syn);
        for (int e = tid; e < E; e += nt) {
            const int v = (GENERAL || tab) ? a.chkVar[e] : 0;
            float x = __uint_as_float(kMinSumCap);  // an unused slot of a general code
            if (!GENERAL || v >= 0) x = tab ? llr[(e < EX ? 0 : n) + v] : lam0;
            msg[e] = x;
        }
        for (int v = tid; v < 2 * n; v += nt) {  // the decisions of N = 0
            int dv;
            const int32_t* ve = sp_var_edges(a, v, dv);
            hd[v] = dv > 0 && (!GENERAL || ve[0] >= 0) && (tab ? llr[v] : lam0) < 0.0f;
        }
        __syncthreads();

        bool actX = true, actZ = true;  // workgroup-uniform
        int itX = 0, itZ = 0;
        for (int it = 0; it < N && (actX || actZ); ++it) {
            const bool last = it == N - 1;
            itX += actX;
            itZ += actZ;
            for (int c = tid; c < m; c += nt) {
                if (c < mX ? !actX : !actZ) continue;
                sp_minsum_check_row<GENERAL, SOFT>(chkDeg, mu, msg, syn, c, dc, alpha);
            }
            __syncthreads();
            for (int v = tid; v < 2 * n; v += nt) {
                if (v >= n ? !actZ : !actX) continue;
                int dv;
                const int32_t* ve = sp_var_edges(a, v, dv);
                bool h;
                sp_minsum_var<MAXDV, GENERAL>(msg, ve, dv, tab ? llr[v] : lam0, last, h);
                hd[v] = h;
            }
            __syncthreads();
            if (STOP == QEC_STOP_REF && it % 10 == 0) {
                bool bx = false, bz = false;
                any_inside(bx, bz);
                const bool anyx = __syncthreads_or(bx), anyz = __syncthreads_or(bz);
                if (actX && !anyx) actX = false;
                if (actZ && !anyz) actZ = false;
            } else if (STOP == QEC_STOP_SYNDROME) {
                bool bx = false, bz = false;
                if constexpr (SOFT) sp_soft_syndrome_fails<GENERAL>(a, syn, hd, bx, bz); else sp_syndrome_fails<GENERAL>(a, syn, hd, bx, bz);
                const bool badx = __syncthreads_or(bx), badz = __syncthreads_or(bz);
                if (actX && !badx) actX = false;
                if (actZ && !badz) actZ = false;
            }
        }

        // ---- the final state: flags from the slots and from the decision bytes, q_final ----
        bool bx = false, bz = false;
        any_inside(bx, bz);
        for (int v = tid; v < 2 * n; v += nt) {
            if (v >= n) a.eZ[b * n + (v - n)] = hd[v]; else a.eX[b * n + v] = hd[v];
        }
        const bool convFailX = __syncthreads_or(bx), convFailZ = __syncthreads_or(bz);
        bool sx = false, sz = false;
        if constexpr (SOFT) sp_soft_syndrome_fails<GENERAL>(a, syn, hd, sx, sz); else sp_syndrome_fails<GENERAL>(a, syn, hd, sx, sz);
        if constexpr (SOFT) sp_soft_store_flips(a, b, syn, fX, fZ);
        const bool synFailX = __syncthreads_or(sx), synFailZ = __syncthreads_or(sz);
        if (a.q != nullptr)
            for (int e = tid; e < E; e += nt) a.q[b * E + e] = (!GENERAL || a.chkVar[e] >= 0) ? msg[e] : 0.0f;
        sp_store_status(a, b, sp_fail_flags(synFailX, synFailZ, convFailX, convFailZ), itX, itZ);
        __syncthreads();  // the workspace is reused by the next syndrome pair
    }
}

// ---- LAYERED: layered min-sum (QEC_OPT_MINSUM_SCHEDULE = 1; DESIGN.md section 2, "The layered min-sum form") -----
// The SERIAL body's layer intervals and two steps with min-sum's arithmetic.  The message array holds R, the
// check->variable LLR of every edge: +0.0f at the start; an unused slot of a general code holds the float K throughout,
// as in the MINSUM body (it changes neither a minimum nor the parity, sp_minsum_check stores it back as K, no fold reads
// it -- the folds walk the variable's real edges only -- and the export writes +0.0f for it).  Per layer interval:
//   * a thread per slot of the layer's checks forms the slot's input, the left fold of the variable's channel LLR and
//     the R of its other checks in ascending check order, and parks it in its own slot (the checks of one colour share
//     no variable, so nobody else reads that slot in this interval); barrier;
//   * a thread per check turns its row into the check's R in place by sp_minsum_check; barrier.
// The posterior pass (thread per variable, the fold over all of the variable's checks) writes the decision bytes and
// folds the inside test into its ballot; it runs where a stop rule looks and once on the final state.  The argument
// block is read as the MINSUM kernels read it (errorProbability = the scalar channel LLR, prior = null or the 2n channel
// LLRs, c0 = alpha) together with the SERIAL kernels' layer tables.  Workspace, grid and workgroup are the scalar plan's.
template <bool GENERAL>
__device__ __forceinline__ float sp_layered_fold(const float* __restrict__ msg, const int32_t* __restrict__ ve, int dv,
                                                 int self, float lam)
{
    float t = lam;
    for (int j = 0; j < dv; ++j) {
        const int ed = ve[j];
        if (GENERAL && ed < 0) break;  // the real entries come first
        if (ed == self) continue;
        t = t + msg[ed];
    }
    return t;
}

template <int STOP, int MAXDC, int MAXDV, bool GENERAL, bool SOFT>
__device__ __forceinline__ void sp_layered_decode(const SparseArgs& a, const uint8_t* __restrict__ chkDeg, uint8_t* ws,
        const float* __restrict__ mu = nullptr, uint8_t* fX = nullptr, uint8_t* fZ = nullptr)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    const int n = a.n, mX = a.mX, mZ = a.mZ, m = mX + mZ, dc = a.dc;
    const int EX = mX * dc, E = m * dc;
    float* msg = reinterpret_cast<float*>(ws);            // E floats
    uint8_t* syn = ws + (size_t)E * sizeof(float);        // m bytes: sX then sZ
    uint8_t* hd = syn + m;                                // 2n bytes: X then Z decisions

    const float lam0 = a.errorProbability, alpha = a.c0;
    const float* llr = a.prior;
    const bool tab = llr != nullptr;  // workgroup-uniform: per-variable channel LLRs or the scalar one
    const int N = a.maxIter < 0 ? 0 : a.maxIter;
    const int LX = a.LX, LZ = a.LZ;
    const int32_t* offX = a.layOff;
    const int32_t* offZ = a.layOff + LX + 1;

    // the posterior pass over the sectors doX / doZ: decision bytes, and whether a posterior is inside the band
    auto posterior = [&](bool doX, bool doZ, bool& bx, bool& bz) {
        for (int v = tid; v < 2 * n; v += nt) {
            const bool z = v >= n;
            if (z ? !doZ : !doX) continue;
            int dv;
            const int32_t* ve = sp_var_edges(a, v, dv);
            if (GENERAL && ve[0] < 0) { hd[v] = 0; continue; }  // a variable in no check decides 0, enters no test
            const float post = sp_layered_fold<GENERAL>(msg, ve, dv, -1, tab ? llr[v] : lam0);
            hd[v] = post < 0.0f;
            if (sp_minsum_inside(post)) { if (z) bz = true; else bx = true; }
        }
    };

    for (long long b = blockIdx.x; b < a.B; b += gridDim.x) {
        if constexpr (SOFT) sp_soft_load_syndromes(a, mu, b, syn); else sp_load_syndromes<GENERAL>(a, chkDeg, b, syn);
        for (int e = tid; e < E; e += nt)
            msg[e] = (!GENERAL || a.chkVar[e] >= 0) ? 0.0f : __uint_as_float(kMinSumCap);
        __syncthreads();

        bool actX = true, actZ = true;  // workgroup-uniform
        int itX = 0, itZ = 0;
        for (int it = 0; it < N && (actX || actZ); ++it) {
            itX += actX;
            itZ += actZ;
            const int layers = max(actX ? LX : 0, actZ ? LZ : 0);
            for (int l = 0; l < layers; ++l) {
                const int x0 = actX && l < LX ? offX[l] : 0, nx = actX && l < LX ? offX[l + 1] - x0 : 0;
                const int z0 = actZ && l < LZ ? offZ[l] : 0, nz = actZ && l < LZ ? offZ[l + 1] - z0 : 0;
                // the slots of the layer's checks, a thread per slot: the input from the slot's variable
                for (int i = tid; i < (nx + nz) * dc; i += nt) {
                    const int j = i / dc, k = i - j * dc;
                    const int c = a.layOrder[j < nx ? x0 + j : z0 + (j - nx)];
                    const int e = c * dc + k, v = a.chkVar[e];
                    if (GENERAL && v < 0) continue;  // an unused slot keeps K
                    const bool z = c >= mX;
                    const int dv = z ? a.dvZ : a.dvX;
                    const int32_t* ve = a.varEdge + (z ? (size_t)n * a.dvX : 0) + (size_t)v * dv;
                    msg[e] = sp_layered_fold<GENERAL>(msg, ve, dv, e, tab ? llr[(z ? n : 0) + v] : lam0);
                }
                __syncthreads();
                // the layer's checks, a thread per check: the row becomes the check's R
                for (int i = tid; i < nx + nz; i += nt) {
                    const int c = a.layOrder[i < nx ? x0 + i : z0 + (i - nx)];
                    sp_minsum_check_row<GENERAL, SOFT>(chkDeg, mu, msg, syn, c, dc, alpha);
                }
                __syncthreads();
            }
            if (STOP == QEC_STOP_REF && it % 10 == 0) {
                bool bx = false, bz = false;
                posterior(actX, actZ, bx, bz);
                const bool anyx = __syncthreads_or(bx), anyz = __syncthreads_or(bz);
                if (actX && !anyx) actX = false;
                if (actZ && !anyz) actZ = false;
            } else if (STOP == QEC_STOP_SYNDROME) {
                bool bx = false, bz = false;
                posterior(actX, actZ, bx, bz);
                __syncthreads();
                bx = bz = false;
                if constexpr (SOFT) sp_soft_syndrome_fails<GENERAL>(a, syn, hd, bx, bz); else sp_syndrome_fails<GENERAL>(a, syn, hd, bx, bz);
                const bool badx = __syncthreads_or(bx), badz = __syncthreads_or(bz);
                if (actX && !badx) actX = false;
                if (actZ && !badz) actZ = false;
            }
        }

        // ---- the final state: decisions, flags, q_final ----
        bool bx = false, bz = false;
        posterior(true, true, bx, bz);
        const bool convFailX = __syncthreads_or(bx), convFailZ = __syncthreads_or(bz);
        for (int v = tid; v < 2 * n; v += nt) {
            if (v >= n) a.eZ[b * n + (v - n)] = hd[v]; else a.eX[b * n + v] = hd[v];
        }
        bool sx = false, sz = false;
        if constexpr (SOFT) sp_soft_syndrome_fails<GENERAL>(a, syn, hd, sx, sz); else sp_syndrome_fails<GENERAL>(a, syn, hd, sx, sz);
        if constexpr (SOFT) sp_soft_store_flips(a, b, syn, fX, fZ);
        const bool synFailX = __syncthreads_or(sx), synFailZ = __syncthreads_or(sz);
        if (a.q != nullptr)
            for (int e = tid; e < E; e += nt) {
                const int v = a.chkVar[e];
                float post = 0.0f;  // an unused slot of a general code
                if (!GENERAL || v >= 0) {
                    const int gv = (e < EX ? 0 : n) + v;
                    int dv;
                    const int32_t* ve = sp_var_edges(a, gv, dv);
                    post = sp_layered_fold<GENERAL>(msg, ve, dv, -1, tab ? llr[gv] : lam0);
                }
                a.q[b * E + e] = post;
            }
        sp_store_status(a, b, sp_fail_flags(synFailX, synFailZ, convFailX, convFailZ), itX, itZ);
        __syncthreads();  // the workspace is reused by the next syndrome pair
    }
}

// ---- RELAY: chained memory min-sum legs (qec_decoder_set_relay; DESIGN.md section 2, "The relay form") -----
// The min-sum body with one fp32 memory M_v per variable and a chain of legs: each leg starts from channel-LLR slots and
// the previous leg's posteriors in M, runs under the call's stop rule counted within the leg, and a leg whose final
// decisions satisfy the syndrome is a solution; the sector ends at its S-th solution or after its last leg and returns
// the lightest solution.  The check update is sp_minsum_check_row, the variable update sp_minsum_var with its folds
// started from the bias b = ((1 - g) lam + g M) + 0.0f (never -0.0f, as that function's padding needs).
// The argument block is read as the MINSUM kernels read it, with the relay's own fields behind it (RelayArgs).  Workspace, grid and
// workgroup are the scalar plan's; the extra state -- M (2n floats) and the best decisions (2n bytes) -- lives in the
// workgroup's slice of a global region (relayWs), where entry v is read and written by v's own thread only (the same
// thread in every pass, v = tid + k nt), so it needs no barrier of its own.
//   * the leg counter, the iteration counter within the leg, the solution count and the best weight of each sector are
//     workgroup-uniform; one loop trip advances every running sector by one iteration, `last` is per sector;
//   * a sector that ends a leg without ending the relay re-initialises its own slots behind the trip's barriers while the
//     other sector's slots stay as they are; a sector that ends the relay keeps the slots and decision bytes of its last
//     executed leg for the flags and the export;
//   * the weight W of a solution is formed only with S > 1 (workgroup-uniform): per-thread sums of w_v over the set
//     decision bytes, added into two static LDS words (integer adds: the order does not matter), no global atomics.
template <int STOP, int MAXDC, int MAXDV, bool GENERAL>
__device__ __forceinline__ void sp_relay_decode(const RelayArgs& a, uint8_t* ws)
{
    __shared__ uint32_t wsum[2];  // the weights of sector X's and sector Z's solution (S > 1)
    const int tid = threadIdx.x, nt = blockDim.x;
    const int n = a.n, mX = a.mX, mZ = a.mZ, m = mX + mZ, dc = a.dc;
    const int EX = mX * dc, E = m * dc;
    float* msg = reinterpret_cast<float*>(ws);            // E floats
    uint8_t* syn = ws + (size_t)E * sizeof(float);        // m bytes: sX then sZ
    uint8_t* hd = syn + m;                                // 2n bytes: X then Z decisions
    uint8_t* rws = a.relayWs + (long long)blockIdx.x * a.relayStride;
    float* mem = reinterpret_cast<float*>(rws);           // M: 2n floats, X then Z
    uint8_t* best = rws + (size_t)2 * n * sizeof(float);  // 2n bytes: the best solution's decisions

    const float lam0 = a.errorProbability, alpha = a.c0;
    const float* llr = a.prior;
    const bool tab = llr != nullptr;  // workgroup-uniform: per-variable channel LLRs or the scalar one
    const int N = a.maxIter < 0 ? 0 : a.maxIter;
    const int L = a.legs, S = a.solutions;
    const bool weigh = S > 1;

    // the slots of sector X (doX) / Z (doZ) at the start of a leg: the channel LLR of the slot's variable
    auto init_slots = [&](bool doX, bool doZ) {
        for (int e = tid; e < E; e += nt) {
            if (e < EX ? !doX : !doZ) continue;
            const int v = (GENERAL || tab) ? a.chkVar[e] : 0;
            float x = __uint_as_float(kMinSumCap);  // an unused slot of a general code
            if (!GENERAL || v >= 0) x = tab ? llr[(e < EX ? 0 : n) + v] : lam0;
            msg[e] = x;
        }
    };

    for (long long b = blockIdx.x; b < a.B; b += gridDim.x) {
        sp_load_syndromes<GENERAL>(a, a.chkDeg, b, syn);
        init_slots(true, true);
        for (int v = tid; v < 2 * n; v += nt) {  // leg 0: M = lambda; the decisions of N = 0
            int dv;
            const int32_t* ve = sp_var_edges(a, v, dv);
            const float lam = tab ? llr[v] : lam0;
            mem[v] = lam;
            hd[v] = dv > 0 && (!GENERAL || ve[0] >= 0) && lam < 0.0f;
        }
        __syncthreads();

        // workgroup-uniform, per sector (0 = X, 1 = Z)
        bool act[2] = {true, true};
        int leg[2] = {0, 0}, k[2] = {0, 0}, its[2] = {0, 0}, sols[2] = {0, 0};
        uint32_t wbest[2] = {0u, 0u};
        while (act[0] || act[1]) {
            bool bad[2] = {true, true};  // SYNDROME: of this trip's decisions
            if (N > 0) {
                const bool lastX = k[0] == N - 1, lastZ = k[1] == N - 1;
                its[0] += act[0];
                its[1] += act[1];
                for (int c = tid; c < m; c += nt) {
                    if (c < mX ? !act[0] : !act[1]) continue;
                    sp_minsum_check_row<GENERAL, false>(a.chkDeg, nullptr, msg, syn, c, dc, alpha);
                }
                __syncthreads();
                for (int v = tid; v < 2 * n; v += nt) {
                    const bool z = v >= n;
                    if (z ? !act[1] : !act[0]) continue;
                    int dv;
                    const int32_t* ve = sp_var_edges(a, v, dv);
                    const float lam = tab ? llr[v] : lam0;
                    const float g = a.gamma[((size_t)(z ? leg[1] : leg[0]) * 2 + z) * n + (z ? v - n : v)];
                    const float t0 = 1.0f - g;
                    const float t1 = t0 * lam;
                    const float t2 = g * mem[v];
                    float bias = t1 + t2;
                    bias = bias + 0.0f;  // -0.0f becomes +0.0f
                    bool h;
                    mem[v] = sp_minsum_var<MAXDV, GENERAL>(msg, ve, dv, bias, z ? lastZ : lastX, h);
                    hd[v] = h;
                }
                __syncthreads();
                k[0] += act[0];
                k[1] += act[1];
            }
            // which sectors end their leg here (the call's stop rule, counted within the leg)
            bool end[2];
            end[0] = act[0] && k[0] == N;
            end[1] = act[1] && k[1] == N;
            if (STOP == QEC_STOP_REF && N > 0) {
                const bool tx = act[0] && (k[0] - 1) % 10 == 0, tz = act[1] && (k[1] - 1) % 10 == 0;
                if (tx || tz) {
                    bool bx = false, bz = false;
                    for (int e = tid; e < E; e += nt) {
                        const bool in = sp_minsum_inside(msg[e]);
                        if (e < EX) bx |= in; else bz |= in;
                    }
                    const bool anyx = __syncthreads_or(bx), anyz = __syncthreads_or(bz);
                    if (tx && !anyx) end[0] = true;
                    if (tz && !anyz) end[1] = true;
                }
            } else if (STOP == QEC_STOP_SYNDROME && N > 0) {
                bool bx = false, bz = false;
                sp_syndrome_fails<GENERAL>(a, syn, hd, bx, bz);
                bad[0] = __syncthreads_or(bx);
                bad[1] = __syncthreads_or(bz);
                if (act[0] && !bad[0]) end[0] = true;
                if (act[1] && !bad[1]) end[1] = true;
            }
            if (!end[0] && !end[1]) continue;

            // ---- the end of a leg: a solution?  the next leg, or the end of the sector's relay ----
            if (STOP != QEC_STOP_SYNDROME || N == 0) {
                bool bx = false, bz = false;
                sp_syndrome_fails<GENERAL>(a, syn, hd, bx, bz);
                bad[0] = __syncthreads_or(bx);
                bad[1] = __syncthreads_or(bz);
            }
            const bool solved[2] = {end[0] && !bad[0], end[1] && !bad[1]};
            uint32_t W[2] = {0u, 0u};
            if (weigh && (solved[0] || solved[1])) {
                if (tid < 2) wsum[tid] = 0u;
                __syncthreads();
                uint32_t wx = 0u, wz = 0u;
                for (int v = tid; v < 2 * n; v += nt) {
                    const bool z = v >= n;
                    if (!(z ? solved[1] : solved[0]) || !hd[v]) continue;
                    const uint32_t w = a.weight != nullptr ? (uint32_t)a.weight[v] : 1u;
                    if (z) wz += w; else wx += w;
                }
                if (wx) atomicAdd(&wsum[0], wx);
                if (wz) atomicAdd(&wsum[1], wz);
                __syncthreads();
                W[0] = wsum[0];
                W[1] = wsum[1];
            }
            bool keep[2], next[2];
            for (int sec = 0; sec < 2; ++sec) {
                keep[sec] = solved[sec] && (sols[sec] == 0 || W[sec] < wbest[sec]);  // ties keep the earlier leg
                if (keep[sec]) wbest[sec] = W[sec];
                sols[sec] += solved[sec];
                const bool done = end[sec] && (sols[sec] == S || leg[sec] == L - 1 || N == 0);
                next[sec] = end[sec] && !done;
                if (done) act[sec] = false;
                if (next[sec]) { ++leg[sec]; k[sec] = 0; }
            }
            if (keep[0] || keep[1])
                for (int v = tid; v < 2 * n; v += nt)
                    if (v >= n ? keep[1] : keep[0]) best[v] = hd[v];
            if (next[0] || next[1]) {
                init_slots(next[0], next[1]);
                __syncthreads();
            }
        }

        // ---- the final state: the last executed leg's slots and decision bytes, the best solution ----
        bool bx = false, bz = false;
        for (int e = tid; e < E; e += nt) {
            const bool in = sp_minsum_inside(msg[e]);
            if (e < EX) bx |= in; else bz |= in;
        }
        for (int v = tid; v < 2 * n; v += nt) {
            const bool z = v >= n;
            const uint8_t h = (z ? sols[1] : sols[0]) ? best[v] : hd[v];
            if (z) a.eZ[b * n + (v - n)] = h; else a.eX[b * n + v] = h;
        }
        const bool convFailX = __syncthreads_or(bx), convFailZ = __syncthreads_or(bz);
        if (a.q != nullptr)
            for (int e = tid; e < E; e += nt) a.q[b * E + e] = (!GENERAL || a.chkVar[e] >= 0) ? msg[e] : 0.0f;
        sp_store_status(a, b, sp_fail_flags(sols[0] == 0, sols[1] == 0, convFailX, convFailZ), its[0], its[1]);
        __syncthreads();  // the workspace is reused by the next syndrome pair
    }
}

// ---- the kernel ----------------------------------------------------------------
// The one entry: the workspace, and the body that BODY names.
template <int STOP, int MAXDC, int MAXDV, bool LDS, bool GENERAL, int BODY>
__global__ __launch_bounds__(kSparseThreads) void bp_sparse_kernel(const SparseArgsOf<BODY> a)
{
    uint8_t* ws = LDS ? sp_lds : a.scratch + (long long)blockIdx.x * a.ws_bytes;
    if constexpr (BODY == kScalar || BODY == kPriors) sp_flood_decode<STOP, MAXDC, MAXDV, GENERAL, BODY == kPriors>(a, ws);
    else if constexpr (BODY == kCorr) sp_corr_decode<STOP, MAXDC, MAXDV, GENERAL>(a, ws);
    else if constexpr (BODY == kSerial) sp_serial_decode<STOP, MAXDC, MAXDV, GENERAL>(a, ws);
    else if constexpr (BODY == kMinSum || BODY == kSoftMinSum)
    {
        if constexpr (BODY == kSoftMinSum) sp_minsum_decode<STOP, MAXDC, MAXDV, GENERAL, true>(a, a.chkDeg, ws, a.mu, a.fX, a.fZ);
        else sp_minsum_decode<STOP, MAXDC, MAXDV, GENERAL, false>(a, a.chkDeg, ws);
    }
    else if constexpr (BODY == kRelay) sp_relay_decode<STOP, MAXDC, MAXDV, GENERAL>(a, ws);
    else if constexpr (BODY == kSoftLayered) sp_layered_decode<STOP, MAXDC, MAXDV, GENERAL, true>(a, a.chkDeg, ws, a.mu, a.fX, a.fZ);
    else sp_layered_decode<STOP, MAXDC, MAXDV, GENERAL, false>(a, a.chkDeg, ws);
}

// ---- plan ------------------------------------------------------------------
// The kernels of one shape, by body and stop rule.
using SparseKernels = const void* [kVariants][3];

template <int STOP, int MAXDC, int MAXDV, bool LDS, bool GENERAL, int... BODY>
static void sparse_kernels_of_stop(SparseKernels& fn, std::integer_sequence<int, BODY...>)
{
    ((fn[BODY][STOP] = reinterpret_cast<const void*>(&bp_sparse_kernel<STOP, MAXDC, MAXDV, LDS, GENERAL, BODY>)), ...);
}

template <int MAXDC, int MAXDV, bool LDS, bool GENERAL>
static void sparse_kernels(SparseKernels& fn)
{
    const std::make_integer_sequence<int, kVariants> bodies;
    sparse_kernels_of_stop<QEC_STOP_REF, MAXDC, MAXDV, LDS, GENERAL>(fn, bodies);
    sparse_kernels_of_stop<QEC_STOP_FIXED, MAXDC, MAXDV, LDS, GENERAL>(fn, bodies);
    sparse_kernels_of_stop<QEC_STOP_SYNDROME, MAXDC, MAXDV, LDS, GENERAL>(fn, bodies);
}

template <int MAXDC, int MAXDV>
static void sparse_kernels_of_shape(bool lds, bool general, SparseKernels& fn)
{
    if (lds) { if (general) sparse_kernels<MAXDC, MAXDV, true, true>(fn); else sparse_kernels<MAXDC, MAXDV, true, false>(fn); }
    else { if (general) sparse_kernels<MAXDC, MAXDV, false, true>(fn); else sparse_kernels<MAXDC, MAXDV, false, false>(fn); }
}

struct SparsePlan {
    int n = 0, mX = 0, mZ = 0, dc = 0, dvX = 0, dvZ = 0;
    bool lds = true;
    long long ws_bytes = 0;
    int grid = 0;
    SparseKernels fn = {};
    // a general code: its degree bytes and its fitted workgroup size
    bool general = false;
    DeviceArray<uint8_t> chkDeg;
    int threads = kSparseThreads;
    // the SERIAL kernels' layer tables: layers = layOrder [mX + mZ], offX [LX + 1], offZ [LZ + 1] (SparseArgs)
    DeviceArray<int32_t> layers;
    int LX = 0, LZ = 0;
    DeviceArray<int32_t> chkVar, varEdge;
    DeviceArray<uint8_t> scratch;
    // the RELAY kernels' state, grid x relay_stride bytes: allocated by the first qec_decoder_set_relay
    // (sparse_plan_relay_reserve), never by a decode call
    DeviceArray<uint8_t> relay_ws;
    long long relay_stride = 0;
    std::string name;
};

// InitIndexArrays (DecoderCPU.h:41-84) for one sector, with the regularity the reference
// assumes checked: row weight dc and column weight dv everywhere.
static bool index_sector(const std::vector<uint8_t>& pcm, int m, int n, int dc, int dv, int edge0, int32_t* chkVar,
                         int32_t* varEdge, std::string& why)
{
    std::vector<int> cnt(n, 0);
    for (int c = 0; c < m; ++c) {
        int k = 0;
        for (int v = 0; v < n; ++v) {
            if (!pcm[(size_t)c * n + v]) continue;
            if (k >= dc || cnt[v] >= dv) { why = "irregular parity-check matrix"; return false; }
            chkVar[(size_t)c * dc + k] = v;
            varEdge[(size_t)v * dv + cnt[v]++] = edge0 + c * dc + k;
            ++k;
        }
        if (k != dc) { why = "irregular parity-check matrix"; return false; }
    }
    for (int v = 0; v < n; ++v)
        if (cnt[v] != dv) { why = "irregular parity-check matrix"; return false; }
    return true;
}

// The padded tables of one sector of a general code (edge id = c D + slot, sector-global through edge0).
static void index_sector_general(const std::vector<uint8_t>& pcm, int m, int n, int D, int dv, int edge0, int32_t* chkVar,
                                 uint8_t* chkDeg, int32_t* varEdge)
{
    std::vector<int> cnt(n, 0);
    for (int c = 0; c < m; ++c) {
        int k = 0;
        for (int v = 0; v < n; ++v) {
            if (!pcm[(size_t)c * n + v]) continue;
            chkVar[(size_t)c * D + k] = v;
            varEdge[(size_t)v * dv + cnt[v]++] = edge0 + c * D + k;
            ++k;
        }
        chkDeg[c] = (uint8_t)k;
    }
}

void sparse_plan_free(void* plan) { delete static_cast<SparsePlan*>(plan); }

const char* sparse_plan_name(const void* plan) { return static_cast<const SparsePlan*>(plan)->name.c_str(); }

// Builds the device tables; returns nullptr (with qec_last_error set) if the code is outside
// what the reference decodes or what this engine instantiates.
void* sparse_plan_create(const Code& c, int device)
{
    const bool general = c.general;
    const int dc = c.stride(), dvX = c.col_stride(0), dvZ = c.col_stride(1), n = c.n, mX = c.mX, mZ = c.mZ;
    if (dc > 32 || dvX > 16 || dvZ > 16) {
        fail(QEC_ERR_UNSUPPORTED, general ? "sparse engine: needs row weights <= 32 and column weights <= 16"
                                          : "sparse engine: needs L <= 32 and J, K <= 16");
        return nullptr;
    }
    const long long m = (long long)mX + mZ, E = m * dc;
    if (general && (E >= (1LL << 31) || 2LL * n >= (1LL << 31))) {
        fail(QEC_ERR_UNSUPPORTED, "sparse engine: code too large");
        return nullptr;
    }
    std::vector<int32_t> chk((size_t)E, -1), ve((size_t)n * (dvX + dvZ), -1);
    std::vector<uint8_t> cdeg((size_t)m, 0);
    std::string why;
    if (general) {
        index_sector_general(c.pcmX, mX, n, dc, dvX, 0, chk.data(), cdeg.data(), ve.data());
        index_sector_general(c.pcmZ, mZ, n, dc, dvZ, mX * dc, chk.data() + (size_t)mX * dc, cdeg.data() + mX,
                             ve.data() + (size_t)n * dvX);
    } else if (!index_sector(c.pcmX, mX, n, dc, dvX, 0, chk.data(), ve.data(), why) ||
        !index_sector(c.pcmZ, mZ, n, dc, dvZ, mX * dc, chk.data() + (size_t)mX * dc, ve.data() + (size_t)n * dvX,
                      why)) {
        fail(QEC_ERR_UNSUPPORTED, "sparse engine: " + why + " (DecoderCPU assumes row weight L and column weight J/K)");
        return nullptr;
    }
    auto* p = new SparsePlan;
    p->general = general;
    p->n = n; p->mX = mX; p->mZ = mZ; p->dc = dc; p->dvX = dvX; p->dvZ = dvZ;
    p->ws_bytes = (E * 4 + m + 2LL * n + 15) / 16 * 16;
    p->lds = p->ws_bytes <= 160 * 1024 - 64;
    const int wdc = dc <= 8 ? 8 : dc <= 16 ? 16 : 32;
    const int wdv = std::max(dvX, dvZ) <= 4 ? 4 : std::max(dvX, dvZ) <= 8 ? 8 : 16;
    // instantiated shapes: (8,4) (16,8) (32,16); pick the smallest that covers the code
    if (wdc <= 8 && wdv <= 4) sparse_kernels_of_shape<8, 4>(p->lds, general, p->fn);
    else if (wdc <= 16 && wdv <= 8) sparse_kernels_of_shape<16, 8>(p->lds, general, p->fn);
    else sparse_kernels_of_shape<32, 16>(p->lds, general, p->fn);
    if (general) {
        // the smallest workgroup that gives the wider pass a thread per node
        const long long wide = std::max<long long>(m, 2LL * n);
        p->threads = wide <= 64 ? 64 : wide <= 128 ? 128 : kSparseThreads;
    }
    // the serial schedule's processing order and layer offsets, as positions in one array over both sectors
    std::vector<int32_t> lay, ordX, offX, ordZ, offZ;
    code_layer_order(c, 0, ordX, offX);
    code_layer_order(c, 1, ordZ, offZ);
    p->LX = (int)offX.size() - 1;
    p->LZ = (int)offZ.size() - 1;
    lay.insert(lay.end(), ordX.begin(), ordX.end());
    for (int32_t r : ordZ) lay.push_back(mX + r);
    lay.insert(lay.end(), offX.begin(), offX.end());
    for (int32_t o : offZ) lay.push_back(mX + o);
    try {
        if (hipSetDevice(device) != hipSuccess) throw std::runtime_error("hipSetDevice");
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
        int per_cu = 1;
        if (p->lds) {
            // every variant takes the same dynamic LDS (the grid stays the scalar kernels')
            for (const auto& variant : p->fn)
                for (const void* f : variant)
                    if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p->ws_bytes) != hipSuccess)
                        throw std::runtime_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize)");
            per_cu = std::max(1, std::min(8, (int)((160 * 1024) / p->ws_bytes)));
            // a general code: the same 32 waves per CU at most, in its fitted workgroups
            if (general) {
                per_cu = std::max(1, std::min(8 * (kSparseThreads / p->threads), (int)((160 * 1024) / p->ws_bytes)));
                // and no more workgroups than the runtime says are resident at once: one beyond that runs its
                // share of the batch alone behind the others
                for (const void* f : p->fn[kScalar]) {
                    int resident = 0;
                    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&resident, f, p->threads, (size_t)p->ws_bytes) ==
                            hipSuccess && resident > 0)
                        per_cu = std::min(per_cu, resident);
                }
            }
        } else {
            per_cu = 4;
        }
        p->grid = cus * per_cu;
        p->chkVar.reserve(chk.size());
        p->varEdge.reserve(ve.size());
        hip_throw(hipMemcpy(p->chkVar.data(), chk.data(), chk.size() * 4, hipMemcpyHostToDevice), "chkVar upload");
        hip_throw(hipMemcpy(p->varEdge.data(), ve.data(), ve.size() * 4, hipMemcpyHostToDevice), "varEdge upload");
        if (general) {
            p->chkDeg.reserve(cdeg.size());
            hip_throw(hipMemcpy(p->chkDeg.data(), cdeg.data(), cdeg.size(), hipMemcpyHostToDevice), "chkDeg upload");
        }
        p->layers.reserve(lay.size());
        hip_throw(hipMemcpy(p->layers.data(), lay.data(), lay.size() * 4, hipMemcpyHostToDevice), "layer table upload");
        if (!p->lds) p->scratch.reserve((size_t)p->grid * p->ws_bytes);
    } catch (const std::exception& ex) {
        delete p;
        fail(QEC_ERR_HIP, std::string("sparse engine: ") + ex.what());
        return nullptr;
    }
    char buf[192];
    if (general)
        snprintf(buf, sizeof buf, "sparse-general %s threads=%d n=%d mX=%d mZ=%d D=%d dv=%d/%d grid=%d (%s)",
                 p->lds ? "lds" : "hbm", p->threads, n, mX, mZ, dc, dvX, dvZ, p->grid, c.describe().c_str());
    else
        snprintf(buf, sizeof buf, "sparse-graph %s n=%d mX=%d mZ=%d dc=%d dv=%d/%d (%s)", p->lds ? "lds" : "hbm", n, mX, mZ,
                 dc, dvX, dvZ, c.describe().c_str());
    p->name = buf;
    return p;
}

const int32_t* sparse_plan_chkvar(const void* plan) { return static_cast<const SparsePlan*>(plan)->chkVar.data(); }
const int32_t* sparse_plan_varedge(const void* plan) { return static_cast<const SparsePlan*>(plan)->varEdge.data(); }

// The RELAY kernels' per-workgroup state (M: 2n floats, the best decisions: 2n bytes); the caller has made the plan's
// device current.  Allocates once.
int sparse_plan_relay_reserve(void* plan)
{
    auto* p = static_cast<SparsePlan*>(plan);
    p->relay_stride = (10LL * p->n + 15) / 16 * 16;
    try {
        p->relay_ws.reserve((size_t)p->grid * p->relay_stride);
    } catch (const std::exception& ex) {
        return fail(QEC_ERR_NOMEM, std::string("sparse engine: relay workspace: ") + ex.what());
    }
    return QEC_OK;
}

int launch_decode_sparse(void* plan, const SparseDecode& d, hipStream_t stream)
{
    auto* p = static_cast<SparsePlan*>(plan);
    if (d.B <= 0) return QEC_OK;
    if (d.corr && d.prior != nullptr && d.cond == nullptr) return fail(QEC_ERR_ARG, "bp_sparse launch: the correlated form needs its conditional tables");
    if (d.serial && d.corr) return fail(QEC_ERR_UNSUPPORTED, "bp_sparse launch: the serial schedule has no correlated form");
    if (d.minsum && (d.corr || d.serial))
        return fail(QEC_ERR_UNSUPPORTED, "bp_sparse launch: min-sum has no correlated form and no serial schedule");
    if (d.minsum && d.prior != nullptr && d.llr == nullptr)
        return fail(QEC_ERR_ARG, "bp_sparse launch: min-sum under priors needs its LLR tables");
    SparseArgs a{};
    a.sX = d.sX; a.sZ = d.sZ; a.eX = d.eX; a.eZ = d.eZ; a.flags = d.flags; a.iters = d.iters; a.q = d.q;
    a.chkVar = p->chkVar.data();
    a.varEdge = p->varEdge.data();
    a.scratch = p->lds ? nullptr : p->scratch.data();
    a.B = d.B;
    a.ws_bytes = p->ws_bytes;
    a.n = p->n; a.mX = p->mX; a.mZ = p->mZ; a.dc = p->dc; a.dvX = p->dvX; a.dvZ = p->dvZ;
    a.errorProbability = d.errorProbability;
    a.maxIter = d.maxIter;
    a.prior = d.prior;
    a.first = d.corr == 2 ? 1 : 0;
    a.c0 = d.c0; a.c1 = d.c1;
    a.cond = d.cond;
    a.layOrder = p->layers.data();
    a.layOff = p->layers.data() + p->mX + p->mZ;
    a.LX = p->LX; a.LZ = p->LZ;
    if (d.minsum) {  // the MINSUM kernels' reading of the argument block (sp_minsum_decode)
        a.errorProbability = d.lam;
        a.prior = d.prior != nullptr ? d.llr : nullptr;
        a.c0 = (float)d.minsum / 256.0f;
    }
    a.chkDeg = p->general ? p->chkDeg.data() : nullptr;
    int variant = d.minsum ? kMinSum : d.serial ? kSerial : d.corr ? kCorr : d.prior ? kPriors : kScalar;
    if (d.minsum && d.gamma != nullptr) {  // min-sum with relay tables: the RELAY kernels
        if (d.legs < 1 || d.solutions < 1 || p->relay_ws.data() == nullptr)
            return fail(QEC_ERR_ARG, "bp_sparse launch: the relay needs its tables and its workspace (qec_decoder_set_relay)");
        variant = kRelay;
    }
    if (d.minsum && d.gamma == nullptr && d.layered)  // plain min-sum under QEC_OPT_MINSUM_SCHEDULE = 1: the LAYERED kernels
        variant = kLayered;
    if (d.mu != nullptr) {  // syndrome priors (qec_decoder_set_syndrome_priors): the SOFT kernels of plain min-sum
        if (!d.minsum || d.gamma != nullptr)
            return fail(QEC_ERR_UNSUPPORTED, "bp_sparse launch: syndrome priors are built for plain min-sum");
        variant = d.layered ? kSoftLayered : kSoftMinSum;
    }
    // the entry's one argument: the block, or the block with the body's own fields behind it (SparseArgsOf)
    RelayArgs ra{a, d.gamma, d.relay_weight, p->relay_ws.data(), p->relay_stride, d.legs, d.solutions};
    SoftArgs sa{a, d.mu, d.fX, d.fZ};
    void* args[] = {variant == kRelay ? static_cast<void*>(&ra) : d.mu != nullptr ? static_cast<void*>(&sa) : static_cast<void*>(&a)};
    const unsigned grid = (unsigned)std::min<long long>(d.B, p->grid);
    (void)hipLaunchKernel(p->fn[variant][d.stop], dim3(grid), dim3(p->threads), args, p->lds ? (size_t)p->ws_bytes : 0, stream);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(QEC_ERR_HIP, std::string("bp_sparse launch: ") + hipGetErrorString(err));
    return QEC_OK;
}

}  // namespace qec
