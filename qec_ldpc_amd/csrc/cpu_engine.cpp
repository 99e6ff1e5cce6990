// CPU engine of libqecldpc.so (qec_decoder_create with device = -1): DecoderCPU's decode
// (QEC_LDPC/DecoderCPU.h:150-390) for hosts without a GPU and for the reference's unmodified
// `DecoderCPU decoder(code)` call site (include/DecoderCPU.h).  Product code: an independent
// implementation over edge-major tables built from the code's parity-check matrices (the
// reference keeps dense n x m message matrices and pointer tables); the oracle in oracle/ is
// never linked.
//
// Edge e = c dc + k is check c's k-th variable in ascending order (InitIndexArrays,
// DecoderCPU.h:41-84); q[e] is the variable->check message, r[e] the check->variable one.
// Arithmetic is DecoderCPU's, operation for operation, in IEEE binary32 (this unit is built
// with -ffp-contract=off and no fast-math): the left-fold products in ascending neighbour
// order, 1.0f - 2.0f*q, 0.5f*(1 +/- t), P1 / (P0 + P1) (Appendix A of SURVEY.md).
// Samples are independent: a batch is split over std::threads, one workspace each (the
// reference's one decoder per OpenMP thread, DecoderCPU.h:419-438).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "qec_internal.h"
#include "qec_near.h"

namespace qec {

namespace {

struct CpuSector {
    int m = 0, dc = 0, dv = 0;
    std::vector<int32_t> chk_var;   // [m][dc] variables of each check, ascending
    std::vector<int32_t> var_edge;  // [n][dv] edges of each variable, ascending check
    // a general code: dc = the slot stride D and dv = the sector's largest column
    // weight, both tables padded with -1, and each node's own degree
    std::vector<uint8_t> chk_deg, var_deg;
    std::vector<int32_t> order;     // the serial schedule's processing order: the checks by (colour, index)
};

struct CpuPlan {
    int n = 0;
    bool general = false;
    CpuSector sec[2];
};

bool build_sector(const std::vector<uint8_t>& pcm, int m, int n, CpuSector& s, std::string& why)
{
    s.m = m;
    s.dc = 0;
    for (int v = 0; v < n; ++v) s.dc += pcm[v] != 0;  // row 0's weight (DecoderCPU.h:69)
    int dv = 0;
    for (int c = 0; c < m; ++c) dv += pcm[(size_t)c * n] != 0;  // column 0's weight (:77)
    s.dv = dv;
    if (s.dc <= 0 || dv <= 0) { why = "empty row or column"; return false; }
    s.chk_var.assign((size_t)m * s.dc, 0);
    s.var_edge.assign((size_t)n * dv, 0);
    std::vector<int> fill(n, 0);
    for (int c = 0; c < m; ++c) {
        int k = 0;
        for (int v = 0; v < n; ++v) {
            if (!pcm[(size_t)c * n + v]) continue;
            if (k == s.dc || fill[v] == dv) { why = "irregular row or column weights"; return false; }
            s.chk_var[(size_t)c * s.dc + k] = v;
            s.var_edge[(size_t)v * dv + fill[v]++] = c * s.dc + k;  // checks visited in ascending order
            ++k;
        }
        if (k != s.dc) { why = "irregular row weights"; return false; }
    }
    for (int v = 0; v < n; ++v)
        if (fill[v] != dv) { why = "irregular column weights"; return false; }
    return true;
}

// The tables of a general code's sector: any row and column weights, slot stride D.
void build_sector_general(const std::vector<uint8_t>& pcm, int m, int n, int D, int dv, CpuSector& s)
{
    s.m = m;
    s.dc = D;
    s.dv = dv;
    s.chk_var.assign((size_t)m * D, -1);
    s.var_edge.assign((size_t)n * dv, -1);
    s.chk_deg.assign(m, 0);
    s.var_deg.assign(n, 0);
    for (int c = 0; c < m; ++c)
        for (int v = 0; v < n; ++v) {
            if (!pcm[(size_t)c * n + v]) continue;
            const int k = s.chk_deg[c]++;
            s.chk_var[(size_t)c * D + k] = v;
            s.var_edge[(size_t)v * dv + s.var_deg[v]++] = c * D + k;  // checks visited in ascending order
        }
}

inline bool outside(float x) { return !(x > 0.01f && x < 0.99f); }  // CheckConvergence, DecoderCPU.h:231-246
inline bool minsum_inside(float x) { return std::fabs(x) < kMinSumInside; }  // the same band as an LLR: |M| < ln 99

struct Work {
    std::vector<float> q, r, post;
    std::vector<uint8_t> e;
    std::vector<uint8_t> f;  // the soft-syndrome form: the measurement decisions of the sector's checks
};

constexpr int kSoftArg = -2;  // the argmin of a check pass when the virtual input holds the first minimum

// The soft-syndrome form: the virtual input mu of a check enters the running minima and the sign
// XOR ahead of the real slots (the outputs do not depend on the position of an input) ...
inline void soft_input(float mu, uint32_t& min1, uint32_t& min2, uint32_t& par, int& arg)
{
    uint32_t b;
    std::memcpy(&b, &mu, sizeof b);
    const uint32_t a = b & 0x7FFFFFFFu;
    par ^= b >> 31;
    if (a < min1) { min2 = min1; min1 = a; arg = kSoftArg; }
    else if (a < min2) min2 = a;
}
// ... and the virtual slot's own output rho = alpha * (the minimum over the real inputs, under the cap) with the sign
// t ^ (the real inputs' signs); returns f = mu + rho < 0
inline bool soft_decision(float mu, uint32_t min1, uint32_t min2, uint32_t par, int arg, float alpha)
{
    uint32_t b, o;
    std::memcpy(&b, &mu, sizeof b);
    const uint32_t mag = arg == kSoftArg ? min2 : min1;
    float rho;
    std::memcpy(&rho, &mag, sizeof rho);
    rho = alpha * rho;
    std::memcpy(&o, &rho, sizeof o);
    o |= (par ^ (b >> 31)) << 31;
    std::memcpy(&rho, &o, sizeof rho);
    const float postm = mu + rho;
    return postm < 0.0f;
}

// The near-hard criterion C(eps0) (qec_near.h) on the messages q after a var pass:
// every message within eps0 of 0 or 1 (nearT: the compare value of eps0), each variable's messages on one
// side of 0.5, and the sides' parity on every check equal to its syndrome entry (an entry other than 0 / 1
// fails, as it fails the syndrome test).
bool near_hard_state(const CpuSector& S, int n, const uint8_t* syn, const float* q, uint32_t nearT)
{
    const int m = S.m, dc = S.dc, dv = S.dv;
    for (size_t k = 0, E = (size_t)m * dc; k < E; ++k) {
        const float t = __builtin_fmaf(-q[k], q[k], q[k]);
        uint32_t b;
        std::memcpy(&b, &t, sizeof b);
        if (b > nearT) return false;
    }
    for (int v = 0; v < n; ++v) {
        const int32_t* ve = S.var_edge.data() + (size_t)v * dv;
        for (int j = 1; j < dv; ++j)
            if ((q[ve[j]] >= 0.5f) != (q[ve[0]] >= 0.5f)) return false;
    }
    for (int c = 0; c < m; ++c) {
        uint32_t x = 0;
        for (int k = 0; k < dc; ++k) x ^= (uint32_t)(q[(size_t)c * dc + k] >= 0.5f);
        if (x != syn[c]) return false;
    }
    return true;
}

// One sector's BeliefPropogation + the Decode post-processing (DecoderCPU.h:249-292, 354-384).
// Returns the iterations executed; e gets the hard decision, conv / syn_ok the flag tests.
// nearT != 0 (fixed / reference stop, no final messages requested): the near-hard jump -- once a state
// meets C(eps0) every later one does, so the post-processing of this state gives the final decisions and
// flags and the count is where the stop rule ends such a sector.
// pri != nullptr (qec_decoder_set_priors): the sector's per-variable priors pi_v take the place of p' -- the
// initial message of v's edges and the start of its two running products; the caller
// then passes nearT = 0 (the jump's lemma is stated for one p').
int decode_sector(const CpuSector& S, int n, const uint8_t* syn, float errorProbability, const float* pri, int N,
                  int stop, Work& w, bool& conv_out, bool& syn_ok, float* q_out, uint32_t nearT)
{
    const int m = S.m, dc = S.dc, dv = S.dv;
    const size_t E = (size_t)m * dc;
    float* q = w.q.data();
    float* r = w.r.data();
    uint8_t* e = w.e.data();
    const float pp = (2.0f / 3.0f) * errorProbability;  // DecoderCPU.h:259
    const float one_minus_pp = 1.0f - pp;
    if (pri)
        for (size_t k = 0; k < E; ++k) q[k] = pri[S.chk_var[k]];
    else
        std::fill(q, q + E, pp);  // InitVarNodes (:135-148, 265-267)
    auto hard_decision = [&]() {
        for (int v = 0; v < n; ++v) {
            bool hd = false;
            for (int j = 0; j < dv; ++j) hd |= q[S.var_edge[(size_t)v * dv + j]] >= 0.5f;  // :354-373
            e[v] = hd;
        }
    };
    auto syndrome_ok = [&]() {
        for (int c = 0; c < m; ++c) {
            uint32_t x = 0;
            for (int k = 0; k < dc; ++k) x ^= e[S.chk_var[(size_t)c * dc + k]];
            if ((x & 1u) != syn[c]) return false;  // exact compare (:381): an entry other than 0/1 never matches
        }
        return true;
    };
    bool conv = false;
    int it = 0;
    for (int iter = 0; iter < N; ++iter) {
        if (stop == QEC_STOP_REF && conv) break;  // :282
        ++it;
        // EqNodeUpdate (:150-186)
        for (int c = 0; c < m; ++c) {
            const float* qc = q + (size_t)c * dc;
            float* rc = r + (size_t)c * dc;
            const bool s = syn[c] != 0;  // truthiness (:178)
            for (int i = 0; i < dc; ++i) {
                float t = 1.0f;
                for (int k = 0; k < dc; ++k)
                    if (k != i) t = t * (1.0f - 2.0f * qc[k]);
                rc[i] = s ? 0.5f * (1.0f + t) : 0.5f * (1.0f - t);
            }
        }
        // VarNodeUpdate (:188-229); the last iteration includes the self message (:216)
        const bool last = iter == N - 1;
        for (int v = 0; v < n; ++v) {
            const int32_t* ve = S.var_edge.data() + (size_t)v * dv;
            const float pv = pri ? pri[v] : pp, omv = pri ? 1.0f - pri[v] : one_minus_pp;
            for (int j = 0; j < dv; ++j) {
                float P0 = omv, P1 = pv;
                for (int k = 0; k < dv; ++k) {
                    if (k == j && !last) continue;
                    const float rk = r[ve[k]];
                    P0 = P0 * (1.0f - rk);
                    P1 = P1 * rk;
                }
                q[ve[j]] = P1 / (P0 + P1);
            }
        }
        if (stop == QEC_STOP_REF) {
            if (iter % 10 == 0) {  // :287-290
                conv = true;
                for (size_t k = 0; k < E && conv; ++k) conv = outside(q[k]);
            }
        }
        if (nearT != 0u && !last && !(stop == QEC_STOP_REF && conv) && near_hard_state(S, n, syn, q, nearT)) {
            // fixed: every iteration counts; reference: the convergence test passes at the next tested iteration
            const int next10 = (iter / 10 + 1) * 10;
            it = (stop == QEC_STOP_REF && next10 < N - 1 ? next10 : N - 1) + 1;
            break;
        }
        if (stop == QEC_STOP_SYNDROME) {
            hard_decision();
            if (syndrome_ok()) break;
        }
    }
    hard_decision();
    bool c_all = true;
    for (size_t k = 0; k < E && c_all; ++k) c_all = outside(q[k]);  // :375-378
    conv_out = c_all;
    syn_ok = syndrome_ok();  // :380-384
    if (q_out) std::memcpy(q_out, q, E * sizeof(float));
    return it;
}

// decode_sector for a general code: the same rules with each node's own degree, over real edges only
// (DESIGN.md section 2).  Unused slots of q stay +0.0f.  No near-hard jump.  pri: as decode_sector's.
int decode_sector_general(const CpuSector& S, int n, const uint8_t* syn, float errorProbability, const float* pri, int N,
                          int stop, Work& w, bool& conv_out, bool& syn_ok, float* q_out)
{
    const int m = S.m, D = S.dc, dvs = S.dv;
    const size_t E = (size_t)m * D;
    float* q = w.q.data();
    float* r = w.r.data();
    uint8_t* e = w.e.data();
    const float pp = (2.0f / 3.0f) * errorProbability;
    const float one_minus_pp = 1.0f - pp;
    for (int c = 0; c < m; ++c)
        for (int k = 0; k < D; ++k)
            q[(size_t)c * D + k] = k < S.chk_deg[c] ? (pri ? pri[S.chk_var[(size_t)c * D + k]] : pp) : 0.0f;
    auto hard_decision = [&]() {
        for (int v = 0; v < n; ++v) {
            bool hd = false;  // a variable in no check decides 0
            for (int j = 0; j < S.var_deg[v]; ++j) hd |= q[S.var_edge[(size_t)v * dvs + j]] >= 0.5f;
            e[v] = hd;
        }
    };
    auto syndrome_ok = [&]() {
        for (int c = 0; c < m; ++c) {
            uint32_t x = 0;
            for (int k = 0; k < S.chk_deg[c]; ++k) x ^= e[S.chk_var[(size_t)c * D + k]];
            if ((x & 1u) != syn[c]) return false;
        }
        return true;
    };
    auto all_outside = [&]() {
        for (int c = 0; c < m; ++c)
            for (int k = 0; k < S.chk_deg[c]; ++k)
                if (!outside(q[(size_t)c * D + k])) return false;
        return true;
    };
    bool conv = false;
    int it = 0;
    for (int iter = 0; iter < N; ++iter) {
        if (stop == QEC_STOP_REF && conv) break;
        ++it;
        for (int c = 0; c < m; ++c) {
            const float* qc = q + (size_t)c * D;
            float* rc = r + (size_t)c * D;
            const int dc = S.chk_deg[c];
            const bool s = syn[c] != 0;
            for (int i = 0; i < dc; ++i) {
                float t = 1.0f;
                for (int k = 0; k < dc; ++k)
                    if (k != i) t = t * (1.0f - 2.0f * qc[k]);
                rc[i] = s ? 0.5f * (1.0f + t) : 0.5f * (1.0f - t);
            }
        }
        const bool last = iter == N - 1;
        for (int v = 0; v < n; ++v) {
            const int32_t* ve = S.var_edge.data() + (size_t)v * dvs;
            const int dv = S.var_deg[v];
            const float pv = pri ? pri[v] : pp, omv = pri ? 1.0f - pri[v] : one_minus_pp;
            for (int j = 0; j < dv; ++j) {
                float P0 = omv, P1 = pv;
                for (int k = 0; k < dv; ++k) {
                    if (k == j && !last) continue;
                    const float rk = r[ve[k]];
                    P0 = P0 * (1.0f - rk);
                    P1 = P1 * rk;
                }
                q[ve[j]] = P1 / (P0 + P1);
            }
        }
        if (stop == QEC_STOP_REF && iter % 10 == 0) conv = all_outside();
        if (stop == QEC_STOP_SYNDROME) {
            hard_decision();
            if (syndrome_ok()) break;
        }
    }
    hard_decision();
    conv_out = all_outside();
    syn_ok = syndrome_ok();
    if (q_out) std::memcpy(q_out, q, E * sizeof(float));
    return it;
}

// One sector under the serial schedule (QEC_OPT_BP_SCHEDULE = 1; DESIGN.md section 2, "The serial schedule"),
// regular and general codes.  r[e] is the check->variable message R of edge e, 0.5f at the start (an unused slot
// +0.0f throughout).  An iteration takes the checks in S.order; check c first forms the variable->check message of
// each of its slots from the other checks' R as they stand, then its own R by EqNodeUpdate.  The posterior of a
// variable is the same product over all its checks; decisions, both stop tests, the flags and q_out are stated
// over the posteriors, and a variable in no check decides 0 and enters no test.
int decode_sector_serial(const CpuSector& S, int n, bool general, const uint8_t* syn, float errorProbability,
                         const float* pri, int N, int stop, Work& w, bool& conv_out, bool& syn_ok, float* q_out)
{
    const int m = S.m, D = S.dc, dvs = S.dv;
    float* q = w.q.data();     // the current check's inputs
    float* r = w.r.data();
    uint8_t* e = w.e.data();
    const float pp = (2.0f / 3.0f) * errorProbability;
    const float one_minus_pp = 1.0f - pp;
    auto cdeg = [&](int c) { return general ? (int)S.chk_deg[c] : D; };
    auto vdeg = [&](int v) { return general ? (int)S.var_deg[v] : dvs; };
    for (int c = 0; c < m; ++c)
        for (int k = 0; k < D; ++k) r[(size_t)c * D + k] = k < cdeg(c) ? 0.5f : 0.0f;
    std::vector<float>& post = w.post;
    post.resize(n);
    bool inside = false;
    auto posterior = [&]() {
        inside = false;
        for (int v = 0; v < n; ++v) {
            const int dv = vdeg(v);
            if (dv == 0) { e[v] = 0; post[v] = 0.0f; continue; }
            const int32_t* ve = S.var_edge.data() + (size_t)v * dvs;
            float P0 = pri ? 1.0f - pri[v] : one_minus_pp, P1 = pri ? pri[v] : pp;
            for (int j = 0; j < dv; ++j) {
                const float rk = r[ve[j]];
                P0 = P0 * (1.0f - rk);
                P1 = P1 * rk;
            }
            post[v] = P1 / (P0 + P1);
            e[v] = post[v] >= 0.5f;
            inside |= !outside(post[v]);
        }
    };
    auto syndrome_ok = [&]() {
        for (int c = 0; c < m; ++c) {
            uint32_t x = 0;
            for (int k = 0; k < cdeg(c); ++k) x ^= e[S.chk_var[(size_t)c * D + k]];
            if ((x & 1u) != syn[c]) return false;
        }
        return true;
    };
    int it = 0;
    for (int iter = 0; iter < N; ++iter) {
        ++it;
        for (int o = 0; o < m; ++o) {
            const int c = S.order[o], dc = cdeg(c);
            float* rc = r + (size_t)c * D;
            for (int k = 0; k < dc; ++k) {
                const int v = S.chk_var[(size_t)c * D + k], self = c * D + k;
                const int32_t* ve = S.var_edge.data() + (size_t)v * dvs;
                float P0 = pri ? 1.0f - pri[v] : one_minus_pp, P1 = pri ? pri[v] : pp;
                for (int j = 0; j < vdeg(v); ++j) {
                    if (ve[j] == self) continue;
                    const float rk = r[ve[j]];
                    P0 = P0 * (1.0f - rk);
                    P1 = P1 * rk;
                }
                q[k] = P1 / (P0 + P1);
            }
            const bool s = syn[c] != 0;
            for (int i = 0; i < dc; ++i) {
                float t = 1.0f;
                for (int k = 0; k < dc; ++k)
                    if (k != i) t = t * (1.0f - 2.0f * q[k]);
                rc[i] = s ? 0.5f * (1.0f + t) : 0.5f * (1.0f - t);
            }
        }
        if (stop == QEC_STOP_REF && iter % 10 == 0) {
            posterior();
            if (!inside) break;
        }
        if (stop == QEC_STOP_SYNDROME) {
            posterior();
            if (syndrome_ok()) break;
        }
    }
    posterior();
    conv_out = !inside;
    syn_ok = syndrome_ok();
    if (q_out)
        for (int c = 0; c < m; ++c)
            for (int k = 0; k < D; ++k)
                q_out[(size_t)c * D + k] = k < cdeg(c) ? post[S.chk_var[(size_t)c * D + k]] : 0.0f;
    return it;
}

// One sector under scaled min-sum in the LLR domain (QEC_OPT_BP_METHOD = 1; DESIGN.md section 2, "The min-sum form"),
// regular and general codes, flooding.  q[e] is the variable->check message of edge e as an LLR (> 0: the bit is 0),
// lam[v] = the channel LLR of variable v (llr, or the scalar lam0).  The loop holds fp32 adds, one fp32 multiply by
// alpha = scale / 256 and integer operations on bit patterns only; every value is finite.
// mu != nullptr (qec_decoder_set_syndrome_priors; DESIGN.md section 2, "The soft-syndrome form"): the channel LLR of each
// check's measurement-error variable, one virtual input of the check; w.f then holds the measurement decisions f_c, which
// enter the syndrome test.  The inside tests stay on the data slots.
int decode_sector_minsum(const CpuSector& S, int n, bool general, const uint8_t* syn, float lam0, const float* llr,
                         int scale, int N, int stop, Work& w, bool& conv_out, bool& syn_ok, float* q_out, const float* mu)
{
    const int m = S.m, D = S.dc, dvs = S.dv;
    const size_t E = (size_t)m * D;
    float* q = w.q.data();
    float* r = w.r.data();
    uint8_t* e = w.e.data();
    const float alpha = (float)scale / 256.0f;
    auto cdeg = [&](int c) { return general ? (int)S.chk_deg[c] : D; };
    auto vdeg = [&](int v) { return general ? (int)S.var_deg[v] : dvs; };
    auto lam = [&](int v) { return llr ? llr[v] : lam0; };
    for (int c = 0; c < m; ++c)
        for (int k = 0; k < D; ++k) q[(size_t)c * D + k] = k < cdeg(c) ? lam(S.chk_var[(size_t)c * D + k]) : 0.0f;
    for (int v = 0; v < n; ++v) e[v] = vdeg(v) > 0 && lam(v) < 0.0f;  // N = 0
    uint8_t* f = nullptr;
    if (mu) {
        w.f.resize(m);
        f = w.f.data();
        for (int c = 0; c < m; ++c) f[c] = mu[c] < 0.0f;  // N = 0
    }
    auto syndrome_ok = [&]() {
        for (int c = 0; c < m; ++c) {
            uint32_t x = f ? f[c] : 0u;
            for (int k = 0; k < cdeg(c); ++k) x ^= e[S.chk_var[(size_t)c * D + k]];
            if ((x & 1u) != syn[c]) return false;
        }
        return true;
    };
    auto all_outside = [&]() {
        for (int c = 0; c < m; ++c)
            for (int k = 0; k < cdeg(c); ++k)
                if (minsum_inside(q[(size_t)c * D + k])) return false;
        return true;
    };
    bool conv = false;
    int it = 0;
    for (int iter = 0; iter < N; ++iter) {
        if (stop == QEC_STOP_REF && conv) break;
        ++it;
        // check update: first minimum, second minimum and argmin of the magnitudes' patterns under the cap, and the
        // XOR of the sign bits, in one pass
        for (int c = 0; c < m; ++c) {
            const float* qc = q + (size_t)c * D;
            float* rc = r + (size_t)c * D;
            const int dc = cdeg(c);
            uint32_t min1 = kMinSumCap, min2 = kMinSumCap, par = syn[c] != 0;
            int arg = -1;
            if (mu) soft_input(mu[c], min1, min2, par, arg);
            for (int k = 0; k < dc; ++k) {
                uint32_t b;
                std::memcpy(&b, qc + k, sizeof b);
                const uint32_t a = b & 0x7FFFFFFFu;
                par ^= b >> 31;
                if (a < min1) { min2 = min1; min1 = a; arg = k; }
                else if (a < min2) min2 = a;
            }
            for (int i = 0; i < dc; ++i) {
                uint32_t b, o;
                std::memcpy(&b, qc + i, sizeof b);
                const uint32_t mag = i == arg ? min2 : min1;
                float f;
                std::memcpy(&f, &mag, sizeof f);
                f = alpha * f;
                std::memcpy(&o, &f, sizeof o);
                o |= (par ^ (b >> 31)) << 31;
                std::memcpy(rc + i, &o, sizeof o);
            }
            if (mu) f[c] = soft_decision(mu[c], min1, min2, par, arg, alpha);
        }
        // variable update: left folds from the channel LLR in ascending check order; the last iteration of the cap
        // writes the posterior to every slot
        const bool last = iter == N - 1;
        for (int v = 0; v < n; ++v) {
            const int32_t* ve = S.var_edge.data() + (size_t)v * dvs;
            const int dv = vdeg(v);
            float post = lam(v);
            for (int k = 0; k < dv; ++k) post = post + r[ve[k]];
            e[v] = dv > 0 && post < 0.0f;
            for (int j = 0; j < dv; ++j) {
                float t = post;
                if (!last) {
                    t = lam(v);
                    for (int k = 0; k < dv; ++k)
                        if (k != j) t = t + r[ve[k]];
                }
                q[ve[j]] = t;
            }
        }
        if (stop == QEC_STOP_REF && iter % 10 == 0) conv = all_outside();
        if (stop == QEC_STOP_SYNDROME && syndrome_ok()) break;
    }
    conv_out = all_outside();
    syn_ok = syndrome_ok();
    if (q_out) std::memcpy(q_out, q, E * sizeof(float));
    return it;
}

// One sector under layered min-sum (QEC_OPT_MINSUM_SCHEDULE = 1; DESIGN.md section 2, "The layered min-sum form"),
// regular and general codes.  r[e] is the check->variable message R of edge e as an LLR, +0.0f at the start (an unused
// slot +0.0f throughout).  An iteration takes the checks in S.order; check c first forms the input of each of its slots
// -- the left fold of the variable's channel LLR and the R of its other checks as they stand -- and then its own R by
// decode_sector_minsum's check update.  The posterior of a variable is the same fold over all its checks; decisions,
// both stop tests, the flags and q_out are stated over the posteriors, and a variable in no check decides 0 and enters
// no test.  There is no special last iteration.  mu: as decode_sector_minsum's; R[c, virtual] is made when c is processed,
// so f_c = mu_c + R[c, virtual] < 0 is kept in w.f from then on (before: mu_c < 0).
int decode_sector_minsum_layered(const CpuSector& S, int n, bool general, const uint8_t* syn, float lam0, const float* llr,
                                 int scale, int N, int stop, Work& w, bool& conv_out, bool& syn_ok, float* q_out,
                                 const float* mu)
{
    const int m = S.m, D = S.dc, dvs = S.dv;
    float* q = w.q.data();  // the current check's inputs
    float* r = w.r.data();
    uint8_t* e = w.e.data();
    const float alpha = (float)scale / 256.0f;
    auto cdeg = [&](int c) { return general ? (int)S.chk_deg[c] : D; };
    auto vdeg = [&](int v) { return general ? (int)S.var_deg[v] : dvs; };
    auto lam = [&](int v) { return llr ? llr[v] : lam0; };
    std::fill(r, r + (size_t)m * D, 0.0f);
    std::vector<float>& post = w.post;
    post.resize(n);
    bool inside = false;
    auto posterior = [&]() {
        inside = false;
        for (int v = 0; v < n; ++v) {
            const int dv = vdeg(v);
            if (dv == 0) { e[v] = 0; post[v] = 0.0f; continue; }
            const int32_t* ve = S.var_edge.data() + (size_t)v * dvs;
            float t = lam(v);
            for (int j = 0; j < dv; ++j) t = t + r[ve[j]];
            post[v] = t;
            e[v] = t < 0.0f;
            inside |= minsum_inside(t);
        }
    };
    uint8_t* f = nullptr;
    if (mu) {
        w.f.resize(m);
        f = w.f.data();
        for (int c = 0; c < m; ++c) f[c] = mu[c] < 0.0f;  // R[c, virtual] = +0.0f
    }
    auto syndrome_ok = [&]() {
        for (int c = 0; c < m; ++c) {
            uint32_t x = f ? f[c] : 0u;
            for (int k = 0; k < cdeg(c); ++k) x ^= e[S.chk_var[(size_t)c * D + k]];
            if ((x & 1u) != syn[c]) return false;
        }
        return true;
    };
    int it = 0;
    for (int iter = 0; iter < N; ++iter) {
        ++it;
        for (int o = 0; o < m; ++o) {
            const int c = S.order[o], dc = cdeg(c);
            float* rc = r + (size_t)c * D;
            uint32_t min1 = kMinSumCap, min2 = kMinSumCap, par = syn[c] != 0;
            int arg = -1;
            if (mu) soft_input(mu[c], min1, min2, par, arg);
            for (int k = 0; k < dc; ++k) {
                const int v = S.chk_var[(size_t)c * D + k], self = c * D + k;
                const int32_t* ve = S.var_edge.data() + (size_t)v * dvs;
                float t = lam(v);
                for (int j = 0; j < vdeg(v); ++j)
                    if (ve[j] != self) t = t + r[ve[j]];
                q[k] = t;
                uint32_t b;
                std::memcpy(&b, &t, sizeof b);
                const uint32_t a = b & 0x7FFFFFFFu;
                par ^= b >> 31;
                if (a < min1) { min2 = min1; min1 = a; arg = k; }
                else if (a < min2) min2 = a;
            }
            for (int i = 0; i < dc; ++i) {
                uint32_t b, o2;
                std::memcpy(&b, q + i, sizeof b);
                const uint32_t mag = i == arg ? min2 : min1;
                float f;
                std::memcpy(&f, &mag, sizeof f);
                f = alpha * f;
                std::memcpy(&o2, &f, sizeof o2);
                o2 |= (par ^ (b >> 31)) << 31;
                std::memcpy(rc + i, &o2, sizeof o2);
            }
            if (mu) f[c] = soft_decision(mu[c], min1, min2, par, arg, alpha);
        }
        if (stop == QEC_STOP_REF && iter % 10 == 0) {
            posterior();
            if (!inside) break;
        }
        if (stop == QEC_STOP_SYNDROME) {
            posterior();
            if (syndrome_ok()) break;
        }
    }
    posterior();
    conv_out = !inside;
    syn_ok = syndrome_ok();
    if (q_out)
        for (int c = 0; c < m; ++c)
            for (int k = 0; k < D; ++k)
                q_out[(size_t)c * D + k] = k < cdeg(c) ? post[S.chk_var[(size_t)c * D + k]] : 0.0f;
    return it;
}

// One sector under the relay form (qec_decoder_set_relay; DESIGN.md section 2, "The relay form"): min-sum legs chained
// through one fp32 memory per variable.  gam: the sector's rows of the tables, leg l at gam + l * gstride; wt: nullptr
// (w_v = 1) or the sector's integer weights.  Leg l starts from channel-LLR slots and the memory of leg l - 1 (leg 0:
// the channel LLRs), runs under the stop rule counted within the leg, and is a solution when its final decisions satisfy
// the syndrome; the sector ends at its S-th solution or after leg L - 1.  w.e holds the best solution (none: the last
// leg's decisions), q_out and conv_out the last executed leg's final state, syn_ok whether there is a solution; returns
// the iterations over all legs.  The check update and the folds are decode_sector_minsum's.
int decode_sector_relay(const CpuSector& S, int n, bool general, const uint8_t* syn, float lam0, const float* llr,
                        int scale, int N, int stop, const float* gam, size_t gstride, int L, int nsol, const int32_t* wt,
                        Work& w, bool& conv_out, bool& syn_ok, float* q_out)
{
    const int m = S.m, D = S.dc, dvs = S.dv;
    const size_t E = (size_t)m * D;
    float* q = w.q.data();
    float* r = w.r.data();
    uint8_t* e = w.e.data();
    w.post.resize(n);
    float* mem = w.post.data();
    std::vector<uint8_t> best;
    const float alpha = (float)scale / 256.0f;
    auto cdeg = [&](int c) { return general ? (int)S.chk_deg[c] : D; };
    auto vdeg = [&](int v) { return general ? (int)S.var_deg[v] : dvs; };
    auto lam = [&](int v) { return llr ? llr[v] : lam0; };
    auto syndrome_ok = [&]() {
        for (int c = 0; c < m; ++c) {
            uint32_t x = 0;
            for (int k = 0; k < cdeg(c); ++k) x ^= e[S.chk_var[(size_t)c * D + k]];
            if ((x & 1u) != syn[c]) return false;
        }
        return true;
    };
    auto all_outside = [&]() {
        for (int c = 0; c < m; ++c)
            for (int k = 0; k < cdeg(c); ++k)
                if (minsum_inside(q[(size_t)c * D + k])) return false;
        return true;
    };
    for (int v = 0; v < n; ++v) {
        mem[v] = lam(v);
        e[v] = vdeg(v) > 0 && lam(v) < 0.0f;  // N = 0
    }
    int total = 0, found = 0;
    uint32_t wbest = 0;
    for (int leg = 0; leg < L; ++leg) {
        const float* g = gam + (size_t)leg * gstride;
        for (int c = 0; c < m; ++c)
            for (int k = 0; k < D; ++k) q[(size_t)c * D + k] = k < cdeg(c) ? lam(S.chk_var[(size_t)c * D + k]) : 0.0f;
        bool conv = false;
        for (int iter = 0; iter < N; ++iter) {
            if (stop == QEC_STOP_REF && conv) break;
            ++total;
            for (int c = 0; c < m; ++c) {
                const float* qc = q + (size_t)c * D;
                float* rc = r + (size_t)c * D;
                const int dc = cdeg(c);
                uint32_t min1 = kMinSumCap, min2 = kMinSumCap, par = syn[c] != 0;
                int arg = -1;
                for (int k = 0; k < dc; ++k) {
                    uint32_t b;
                    std::memcpy(&b, qc + k, sizeof b);
                    const uint32_t a = b & 0x7FFFFFFFu;
                    par ^= b >> 31;
                    if (a < min1) { min2 = min1; min1 = a; arg = k; }
                    else if (a < min2) min2 = a;
                }
                for (int i = 0; i < dc; ++i) {
                    uint32_t b, o;
                    std::memcpy(&b, qc + i, sizeof b);
                    const uint32_t mag = i == arg ? min2 : min1;
                    float f;
                    std::memcpy(&f, &mag, sizeof f);
                    f = alpha * f;
                    std::memcpy(&o, &f, sizeof o);
                    o |= (par ^ (b >> 31)) << 31;
                    std::memcpy(rc + i, &o, sizeof o);
                }
            }
            const bool last = iter == N - 1;
            for (int v = 0; v < n; ++v) {
                const int32_t* ve = S.var_edge.data() + (size_t)v * dvs;
                const int dv = vdeg(v);
                if (dv == 0) { e[v] = 0; continue; }  // no check: decides 0, no memory
                const float t0 = 1.0f - g[v];
                const float t1 = t0 * lam(v);
                const float t2 = g[v] * mem[v];
                float bias = t1 + t2;
                bias = bias + 0.0f;  // -0.0f becomes +0.0f
                float post = bias;
                for (int k = 0; k < dv; ++k) post = post + r[ve[k]];
                e[v] = post < 0.0f;
                mem[v] = post;
                for (int j = 0; j < dv; ++j) {
                    float t = post;
                    if (!last) {
                        t = bias;
                        for (int k = 0; k < dv; ++k)
                            if (k != j) t = t + r[ve[k]];
                    }
                    q[ve[j]] = t;
                }
            }
            if (stop == QEC_STOP_REF && iter % 10 == 0) conv = all_outside();
            if (stop == QEC_STOP_SYNDROME && syndrome_ok()) break;
        }
        if (syndrome_ok()) {  // a solution: the lightest so far wins, ties keep the earlier leg
            uint32_t W = 0;
            for (int v = 0; v < n; ++v)
                if (e[v]) W += wt ? (uint32_t)wt[v] : 1u;
            if (found == 0 || W < wbest) { wbest = W; best.assign(e, e + n); }
            ++found;
        }
        if (found == nsol || N == 0) break;
    }
    conv_out = all_outside();
    syn_ok = found > 0;
    if (q_out) std::memcpy(q_out, q, E * sizeof(float));
    if (found) std::memcpy(e, best.data(), n);
    return total;
}

}  // namespace

// The channel LLR of the min-sum form (qec_minsum_llr): (float) log((1 - pi) / pi), the float prior taken exactly to
// double and the result rounded once, clamped to [-2^30, +2^30]; pi <= 0 gives +2^30, pi >= 1 gives -2^30 and
// pi = 1/2 gives +0.0f (never -0.0f: the kernels' padding relies on that).  Both engines decode with these values.
float minsum_llr(float prior)
{
    const double pi = (double)prior;
    if (!(pi > 0.0)) return kMinSumLlrMax;
    if (pi >= 1.0) return -kMinSumLlrMax;
    const float l = (float)std::log((1.0 - pi) / pi);
    return std::min(kMinSumLlrMax, std::max(-kMinSumLlrMax, l)) + 0.0f;
}

void* cpu_plan_create(const Code& c)
{
    auto* p = new CpuPlan;
    p->n = c.n;
    if (c.general) {
        if (c.D > 255 || c.dvX > 255 || c.dvZ > 255) {
            delete p;
            fail(QEC_ERR_UNSUPPORTED, "CPU engine: row and column weights above 255");
            return nullptr;
        }
        p->general = true;
        build_sector_general(c.pcmX, c.mX, c.n, c.D, c.dvX, p->sec[0]);
        build_sector_general(c.pcmZ, c.mZ, c.n, c.D, c.dvZ, p->sec[1]);
        std::vector<int32_t> off;
        for (int sec = 0; sec < 2; ++sec) code_layer_order(c, sec, p->sec[sec].order, off);
        return p;
    }
    std::string why;
    if (!build_sector(c.pcmX, c.mX, c.n, p->sec[0], why) || !build_sector(c.pcmZ, c.mZ, c.n, p->sec[1], why)) {
        delete p;
        fail(QEC_ERR_UNSUPPORTED, "CPU engine: " + why + " (DecoderCPU assumes regular degrees)");
        return nullptr;
    }
    std::vector<int32_t> off;
    for (int sec = 0; sec < 2; ++sec) code_layer_order(c, sec, p->sec[sec].order, off);
    return p;
}

void cpu_plan_free(void* plan) { delete static_cast<CpuPlan*>(plan); }

int cpu_threads()
{
    const unsigned h = std::thread::hardware_concurrency();
    return h ? (int)h : 1;
}

// The scalar tables of the correlated form (qec_correlated_priors): P(other bit | this bit clear) and
// P(other bit | this bit set) under depolarising noise of strength p, every operation in fp32 (this unit is
// built with -ffp-contract=off).  Both engines decode with these values.
void correlated_priors(float p, float* c0, float* c1)
{
    const float marginal = 2.0f / 3.0f * p;
    const float clear = 1.0f - marginal;
    *c0 = (p / 3.0f) / clear;
    *c1 = 0.5f;
}

// Batched Decode on host buffers; outputs in byte form (eX, eZ, flags) and/or packed records.
// prior: nullptr, or the handle's priors (n floats of sector X, then n of sector Z); p is then unused.
// corr (QEC_OPT_CORRELATED): 0, or 1 / 2 = the correlated form with first sector X / Z -- the first sector as
// under 0, the second by the prior form with pi_v = d[v] ? c1[v] : c0[v], d the first sector's estimate; cond
// (with prior) = the tables c0_X [n], c1_X [n], c0_Z [n], c1_Z [n], without prior the pair correlated_priors(p).
// The near-hard jump never fires for the second sector.
// serial (QEC_OPT_BP_SCHEDULE): 1 = the serial schedule (decode_sector_serial; no near-hard jump, never with corr).
// minsum (QEC_OPT_BP_METHOD = 1): 0, or the scale k of scaled min-sum (decode_sector_minsum; flooding, no near-hard
// jump, never with corr or serial); llr (with prior) = the handle's channel LLR tables, sector X [n] then Z [n],
// without prior the scalar minsum_llr(p').
// gamma (with minsum; qec_decoder_set_relay): nullptr, or the relay tables [legs][sector][n] for decode_sector_relay, with
// solutions = S and weight = nullptr (w_v = 1) or the integer weights of the priors, sector X [n] then Z [n].
// layered (QEC_OPT_MINSUM_SCHEDULE; with minsum and without gamma): 1 = layered min-sum (decode_sector_minsum_layered).
// mu (with minsum and without gamma; qec_decoder_set_syndrome_priors): nullptr, or the measurement-error LLRs, sector X
// [mX] then Z [mZ]; fX / fZ (nullable, [B][mX] / [B][mZ]) receive the measurement decisions, zeros without mu.
int cpu_decode_batch(void* plan, const uint8_t* sX, const uint8_t* sZ, long long B, float p, int maxIter, int stop,
                     uint8_t* eX, uint8_t* eZ, uint8_t* flags, uint8_t* rec, int32_t* iters, float* qf, int threads,
                     bool near_hard, const float* prior, int corr, const float* cond, int serial, int minsum,
                     const float* llr, const float* gamma, int legs, int solutions, const int32_t* weight, int layered,
                     const float* mu, uint8_t* fX, uint8_t* fZ)
{
    const CpuPlan& P = *static_cast<const CpuPlan*>(plan);
    const int n = P.n, nb = (n + 7) / 8;
    const int mX = P.sec[0].m, mZ = P.sec[1].m;
    const size_t qper = (size_t)mX * P.sec[0].dc + (size_t)mZ * P.sec[1].dc;
    // near-hard jump (QEC_OPT_NEAR_HARD_JUMP): per-sector compare values for this p', as the kernels' launch
    uint32_t nearT[2] = {0u, 0u};
    if (near_hard && !minsum && !prior && !P.general && qf == nullptr && stop != QEC_STOP_SYNDROME)
        for (int sec = 0; sec < 2; ++sec) nearT[sec] = near_hard_threshold((2.0f / 3.0f) * p, P.sec[sec].dv, P.sec[sec].dc).T;
    if (corr && prior && !cond) return fail(QEC_ERR_ARG, "CPU engine: the correlated form needs its conditional tables");
    if (serial && corr) return fail(QEC_ERR_UNSUPPORTED, "CPU engine: the serial schedule has no correlated form");
    if (minsum && (corr || serial))
        return fail(QEC_ERR_UNSUPPORTED, "CPU engine: min-sum has no correlated form and no serial schedule");
    if (minsum && prior && !llr) return fail(QEC_ERR_ARG, "CPU engine: min-sum under priors needs its LLR tables");
    if (mu && (!minsum || gamma))
        return fail(QEC_ERR_UNSUPPORTED, "CPU engine: syndrome priors are built for plain min-sum");
    const float lam0 = minsum_llr(2.0f / 3.0f * p);
    float sc0 = 0.0f, sc1 = 0.0f;
    if (corr) correlated_priors(p, &sc0, &sc1);
    if (threads <= 0) threads = cpu_threads();
    threads = (int)std::max<long long>(1, std::min<long long>(threads, B));
    auto run = [&](long long lo, long long hi) {
        Work w;
        std::vector<uint8_t> first(corr ? n : 0);  // the first sector's estimate
        std::vector<float> pi(corr ? n : 0);       // the second sector's priors of this sample
        const size_t E = std::max((size_t)mX * P.sec[0].dc, (size_t)mZ * P.sec[1].dc);
        w.q.resize(E);
        w.r.resize(E);
        w.e.resize(n);
        for (long long b = lo; b < hi; ++b) {
            uint8_t f = 0;
            for (int pass = 0; pass < 2; ++pass) {
                const int sec = corr == 2 ? 1 - pass : pass;
                const CpuSector& S = P.sec[sec];
                bool conv = false, ok = false;
                float* qo = qf ? qf + b * qper + (sec ? (size_t)mX * P.sec[0].dc : 0) : nullptr;
                const uint8_t* syn = sec ? sZ + b * mZ : sX + b * mX;
                const float* pri = prior ? prior + (size_t)sec * n : nullptr;
                const bool second = corr && pass == 1;
                const float* mus = mu ? mu + (sec ? mX : 0) : nullptr;
                if (second) {
                    const float* t0 = cond ? cond + (size_t)sec * 2 * n : nullptr;
                    for (int v = 0; v < n; ++v) pi[v] = first[v] ? (cond ? t0[n + v] : sc1) : (cond ? t0[v] : sc0);
                    pri = pi.data();
                }
                const int it = minsum && gamma ? decode_sector_relay(S, n, P.general, syn, lam0, prior ? llr + (size_t)sec * n : nullptr,
                                                                     minsum, maxIter, stop, gamma + (size_t)sec * n, 2 * (size_t)n, legs,
                                                                     solutions, weight ? weight + (size_t)sec * n : nullptr, w, conv,
                                                                     ok, qo)
                               : minsum && layered ? decode_sector_minsum_layered(S, n, P.general, syn, lam0,
                                                                                  prior ? llr + (size_t)sec * n : nullptr, minsum,
                                                                                  maxIter, stop, w, conv, ok, qo, mus)
                               : minsum ? decode_sector_minsum(S, n, P.general, syn, lam0, prior ? llr + (size_t)sec * n : nullptr,
                                                             minsum, maxIter, stop, w, conv, ok, qo, mus)
                               : serial ? decode_sector_serial(S, n, P.general, syn, p, pri, maxIter, stop, w, conv, ok, qo)
                               : P.general ? decode_sector_general(S, n, syn, p, pri, maxIter, stop, w, conv, ok, qo)
                                           : decode_sector(S, n, syn, p, pri, maxIter, stop, w, conv, ok, qo,
                                                           second ? 0u : nearT[sec]);
                if (corr && pass == 0) std::memcpy(first.data(), w.e.data(), n);
                if (uint8_t* fo = sec ? fZ : fX) {
                    if (mu) std::memcpy(fo + b * S.m, w.f.data(), S.m);
                    else std::memset(fo + b * S.m, 0, S.m);
                }
                if (!ok) f |= sec ? QEC_SYNDROME_FAIL_Z : QEC_SYNDROME_FAIL_X;
                if (!conv) f |= sec ? QEC_CONVERGENCE_FAIL_Z : QEC_CONVERGENCE_FAIL_X;
                if (iters) iters[2 * b + sec] = it;
                if (rec) {
                    uint8_t* o = rec + b * (2 * nb + 1) + sec * nb;
                    std::memset(o, 0, nb);
                    for (int v = 0; v < n; ++v) o[v >> 3] |= (uint8_t)(w.e[v] << (v & 7));
                } else {
                    std::memcpy((sec ? eZ : eX) + b * n, w.e.data(), n);
                }
            }
            if (rec) rec[b * (2 * nb + 1) + 2 * nb] = f;
            else flags[b] = f;
        }
    };
    if (threads == 1) {
        run(0, B);
    } else {
        std::vector<std::thread> th;
        for (int t = 0; t < threads; ++t) th.emplace_back(run, B * t / threads, B * (t + 1) / threads);
        for (auto& x : th) x.join();
    }
    return QEC_OK;
}

}  // namespace qec
