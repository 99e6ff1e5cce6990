// OSD-0 and the combination sweep on the host (DESIGN.md sections 1.2, 1.3): the CPU engine's
// post-processing stage and the in-library cross-check of the kernel (osd.hip).  Plain C++ on
// bit-packed rows; no GPU.
#include <algorithm>
#include <cmath>
#include <thread>

#include "qec_osd.h"

namespace qec {

namespace {

void build_sector(const std::vector<uint8_t>& pcm, int m, int n, int L, size_t qbase, OsdSector& S)
{
    S.m = m;
    S.n = n;
    S.W = (n + 1 + 31) / 32;
    S.H.assign((size_t)m * S.W, 0u);
    S.qpos.assign(n, -1);
    for (int c = 0; c < m; ++c) {
        int slot = 0;  // q_final: [check][slot], slots in ascending variable order
        for (int v = 0; v < n; ++v) {
            if (!pcm[(size_t)c * n + v]) continue;
            S.H[(size_t)c * S.W + (v >> 5)] |= 1u << (v & 31);
            if (S.qpos[v] < 0 && slot < L) S.qpos[v] = (int32_t)(qbase + (size_t)c * L + slot);
            ++slot;
        }
    }
    // rank(H): plain elimination on a copy, columns left to right
    std::vector<uint32_t> A = S.H;
    int r = 0;
    for (int v = 0; v < n && r < m; ++v) {
        const int w = v >> 5;
        const uint32_t bit = 1u << (v & 31);
        int p = -1;
        for (int c = r; c < m; ++c)
            if (A[(size_t)c * S.W + w] & bit) { p = c; break; }
        if (p < 0) continue;
        if (p != r)
            for (int k = 0; k < S.W; ++k) std::swap(A[(size_t)p * S.W + k], A[(size_t)r * S.W + k]);
        for (int c = r + 1; c < m; ++c)
            if (A[(size_t)c * S.W + w] & bit)
                for (int k = w; k < S.W; ++k) A[(size_t)c * S.W + k] ^= A[(size_t)r * S.W + k];
        ++r;
    }
    S.rank = r;
}

}  // namespace

void osd_plan_build(const Code& c, OsdPlan& out)
{
    const int L = c.stride();  // slots per check of the q_final layout (a general code: D)
    out.qn = (size_t)(c.mX + c.mZ) * L;
    build_sector(c.pcmX, c.mX, c.n, L, 0, out.sec[0]);
    build_sector(c.pcmZ, c.mZ, c.n, L, (size_t)c.mX * L, out.sec[1]);
}

int32_t osd_weight(float prior)
{
    const double pi = (double)prior;
    if (pi >= 0.5) return 0;
    if (pi == 0.0) return kOsdMaxWeight;
    return (int32_t)std::min<long long>(kOsdMaxWeight, std::llrint(16.0 * std::log2((1.0 - pi) / pi)));
}

bool osd_host_sector(const OsdSector& S, const float* q, const uint8_t* s, uint8_t* e, int order_cs, bool* swept,
                     const int32_t* wt_tab, bool llr)
{
    if (swept) *swept = false;
    const int m = S.m, n = S.n, W = S.W;
    // a syndrome entry other than 0 or 1 can never be reproduced (the reference compares exact values)
    for (int c = 0; c < m; ++c)
        if (s[c] > 1) return false;
    std::vector<uint32_t> key(n);
    std::vector<int> order(n);
    for (int v = 0; v < n; ++v) {
        uint32_t bits = llr ? 0u : kOsdHalf;
        if (S.qpos[v] >= 0) std::memcpy(&bits, q + S.qpos[v], sizeof bits);
        key[v] = llr ? osd_key_llr(bits) : osd_key(bits);
        order[v] = v;
    }
    std::sort(order.begin(), order.end(), [&](int a, int b) { return key[a] != key[b] ? key[a] > key[b] : a < b; });
    std::vector<uint32_t> A = S.H;  // [H | s]
    const int sw = n >> 5;
    const uint32_t sbit = 1u << (n & 31);
    for (int c = 0; c < m; ++c)
        if (s[c]) A[(size_t)c * W + sw] |= sbit;
    std::vector<int> pivcol(m, -1);
    int npiv = 0;
    for (int t = 0; t < n && npiv < S.rank; ++t) {
        const int v = order[t], w = v >> 5;
        const uint32_t bit = 1u << (v & 31);
        int p = -1;
        for (int c = 0; c < m; ++c)
            if (pivcol[c] < 0 && (A[(size_t)c * W + w] & bit)) { p = c; break; }
        if (p < 0) continue;  // dependent on the pivots chosen so far
        const uint32_t* pr = &A[(size_t)p * W];
        for (int c = 0; c < m; ++c)
            if (c != p && (A[(size_t)c * W + w] & bit)) {
                uint32_t* row = &A[(size_t)c * W];
                for (int k = 0; k < W; ++k) row[k] ^= pr[k];
            }
        pivcol[p] = v;
        ++npiv;
    }
    // the rows without a pivot are zero in H now: s is in the column space iff they are zero in s too
    for (int c = 0; c < m; ++c)
        if (pivcol[c] < 0 && (A[(size_t)c * W + sw] & sbit)) return false;
    // section 1.3: T = the non-pivot columns in the walk's order; a candidate flips a set F of them, and
    // its weight is |F| plus the pivot rows whose s' bit, XOR their bits in the columns of F, is set
    // (section 1.4, with a weight table: each flip counts its qubit's weight instead of one)
    int F[2] = {-1, -1};
    if (order_cs > 0) {
        std::vector<uint8_t> is_piv(n, 0);
        for (int c = 0; c < m; ++c)
            if (pivcol[c] >= 0) is_piv[pivcol[c]] = 1;
        std::vector<int> T;
        for (int t = 0; t < n; ++t)
            if (!is_piv[order[t]]) T.push_back(order[t]);
        const int f = (int)T.size(), lam = std::min(order_cs, f);
        auto bit_at = [&](int c, int v) { return (A[(size_t)c * W + (v >> 5)] >> (v & 31)) & 1u; };
        auto weight = [&](int a, int b) {
            auto cost = [&](int v) { return wt_tab ? (int)wt_tab[v] : 1; };
            int wt = (a >= 0 ? cost(a) : 0) + (b >= 0 ? cost(b) : 0);
            for (int c = 0; c < m; ++c) {
                if (pivcol[c] < 0) continue;
                uint32_t x = bit_at(c, n);
                if (a >= 0) x ^= bit_at(c, a);
                if (b >= 0) x ^= bit_at(c, b);
                if (x) wt += cost(pivcol[c]);
            }
            return wt;
        };
        // candidates in index order, a strictly lighter one replaces the best: the first minimum wins
        int best = weight(-1, -1);
        for (int j = 0; j < f; ++j) {
            const int wt = weight(T[j], -1);
            if (wt < best) { best = wt; F[0] = T[j]; F[1] = -1; if (swept) *swept = true; }
        }
        for (int i = 0; i < lam; ++i)
            for (int j = i + 1; j < lam; ++j) {
                const int wt = weight(T[i], T[j]);
                if (wt < best) { best = wt; F[0] = T[i]; F[1] = T[j]; if (swept) *swept = true; }
            }
    }
    std::memset(e, 0, n);
    for (int c = 0; c < m; ++c) {
        if (pivcol[c] < 0) continue;
        uint32_t x = A[(size_t)c * W + sw] & sbit ? 1u : 0u;
        for (int k = 0; k < 2; ++k)
            if (F[k] >= 0) x ^= (A[(size_t)c * W + (F[k] >> 5)] >> (F[k] & 31)) & 1u;
        e[pivcol[c]] = (uint8_t)x;
    }
    for (int k = 0; k < 2; ++k)
        if (F[k] >= 0) e[F[k]] = 1;
    return true;
}

long long osd_host_batch(const OsdPlan& P, const uint8_t* sX, const uint8_t* sZ, long long B, const float* q,
                         uint8_t* eX, uint8_t* eZ, uint8_t* flags, int threads, int order, long long* swept,
                         const int32_t* w, bool llr)
{
    if (swept) *swept = 0;
    if (B <= 0) return 0;
    if (threads <= 0) {
        const unsigned h = std::thread::hardware_concurrency();
        threads = h ? (int)h : 1;
    }
    threads = (int)std::max<long long>(1, std::min<long long>(threads, B));
    std::vector<long long> fixed(threads, 0), cs(threads, 0);
    auto run = [&](int t, long long lo, long long hi) {
        for (long long b = lo; b < hi; ++b)
            for (int sec = 0; sec < 2; ++sec) {
                const uint8_t fbit = sec ? QEC_SYNDROME_FAIL_Z : QEC_SYNDROME_FAIL_X;
                if (!(flags[b] & fbit)) continue;
                const OsdSector& S = P.sec[sec];
                bool sw = false;
                if (osd_host_sector(S, q + (size_t)b * P.qn, (sec ? sZ : sX) + (size_t)b * S.m,
                                    (sec ? eZ : eX) + (size_t)b * S.n, order, &sw,
                                    w ? w + (size_t)sec * S.n : nullptr, llr)) {
                    flags[b] &= (uint8_t)~fbit;
                    ++fixed[t];
                    cs[t] += sw;
                }
            }
    };
    if (threads == 1) {
        run(0, 0, B);
    } else {
        std::vector<std::thread> th;
        for (int t = 0; t < threads; ++t) th.emplace_back(run, t, B * t / threads, B * (t + 1) / threads);
        for (auto& x : th) x.join();
    }
    long long total = 0;
    for (long long f : fixed) total += f;
    if (swept)
        for (long long x : cs) *swept += x;
    return total;
}

}  // namespace qec
