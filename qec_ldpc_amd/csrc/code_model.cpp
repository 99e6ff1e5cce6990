// Host-side code model: the Quantum_LDPC_Code loader, the QC_LDPC_CSS generator,
// circulant extraction, syndromes, the I-P logical check and the reference's
// MSVC-compatible error sampler.  Product code (no oracle dependency).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>

#include "qec_internal.h"

namespace qec {

namespace {
thread_local std::string g_last_error;

// `stream >> x` until the stream fails (Quantum_LDPC_Code.h:28-41).  Values past
// the matrix size are ignored (the reference would write past its buffer).
void parse_matrix(const std::string& line, std::vector<uint8_t>& dst, size_t cap)
{
    dst.assign(cap, 0);
    const char* p = line.data();
    const char* end = p + line.size();
    size_t idx = 0;
    while (p < end) {
        while (p < end && (*p == ' ' || *p == '\t' || *p == '\r' || *p == '\v' || *p == '\f')) ++p;
        if (p >= end) break;
        bool neg = false;
        if (*p == '-' || *p == '+') { neg = (*p == '-'); ++p; }
        if (p >= end || *p < '0' || *p > '9') break;
        long v = 0;
        while (p < end && *p >= '0' && *p <= '9') v = v * 10 + (*p++ - '0');
        if (idx < cap) dst[idx] = (uint8_t)((neg ? -v : v) != 0);
        ++idx;
    }
}

long pow_mod(long base, long e, long P)
{
    long t = 1;
    for (long i = 0; i < e; ++i) t = (t * base) % P;
    return t;
}
}  // namespace

void set_error(const std::string& msg) { g_last_error = msg; }
int fail(int status, const std::string& msg)
{
    g_last_error = msg;
    return status;
}
const char* last_error_cstr() { return g_last_error.c_str(); }

std::string Code::describe() const
{
    std::ostringstream s;
    if (general) {
        s << "[[n=" << n << ",k=" << k << "]]";
        return s.str();
    }
    s << "[J=" << J << ",K=" << K << ",L=" << L << ",P=" << P << ",s=" << sigma << ",t=" << tau
      << "][[n=" << n << ",k=" << (mZ - mX) << "]]";
    return s.str();
}

// A block is a circulant permutation matrix if row i has its single 1 at column (E + i) mod P.
static bool extract_shifts(const std::vector<uint8_t>& pcm, int R, int L, int P, std::vector<int>& E)
{
    const int n = L * P;
    E.assign((size_t)R * L, 0);
    for (int r = 0; r < R; ++r)
        for (int l = 0; l < L; ++l) {
            int e0 = -1;
            for (int c = 0; c < P; ++c)
                if (pcm[(size_t)(r * P) * n + l * P + c]) {
                    if (e0 >= 0) return false;
                    e0 = c;
                }
            if (e0 < 0) return false;
            for (int i = 0; i < P; ++i)
                for (int c = 0; c < P; ++c) {
                    const bool one = pcm[(size_t)(r * P + i) * n + l * P + c] != 0;
                    if (one != (c == (e0 + i) % P)) return false;
                }
            E[(size_t)r * L + l] = e0;
        }
    return true;
}

void finalize_code(Code& c)
{
    if (!c.general) {
        c.n = c.L * c.P;
        c.mX = c.J * c.P;
        c.mZ = c.K * c.P;
        c.is_qc = extract_shifts(c.pcmX, c.J, c.L, c.P, c.EX) && extract_shifts(c.pcmZ, c.K, c.L, c.P, c.EZ);
    }
    if (!c.is_qc) { c.EX.clear(); c.EZ.clear(); }
    c.imp_rows.clear();
    c.imp_words = 0;
    if (!c.imp.empty()) {
        const int N2 = 2 * c.n;
        c.imp_words = (N2 + 63) / 64;
        std::vector<uint64_t> row(c.imp_words);
        for (int i = 0; i < N2; ++i) {
            std::fill(row.begin(), row.end(), 0);
            bool any = false;
            for (int j = 0; j < N2; ++j)
                if (c.imp[(size_t)i * N2 + j]) { row[j >> 6] |= 1ull << (j & 63); any = true; }
            if (any) c.imp_rows.insert(c.imp_rows.end(), row.begin(), row.end());
        }
        // the same test column by column: (I-P) r != 0 iff the XOR of the columns of I-P at the set
        // bits of r, restricted to its non-zero rows, is non-zero.  A decoded residual is almost
        // always 0 or sparse, so the device kernels touch a few columns instead of every row.
        const int nrows = c.imp_words ? (int)(c.imp_rows.size() / c.imp_words) : 0;
        c.imp_col_words = (nrows + 63) / 64;
        c.imp_cols.assign((size_t)N2 * c.imp_col_words, 0);
        int k = 0;
        for (int i = 0; i < N2; ++i) {
            bool any = false;
            for (int j = 0; j < N2 && !any; ++j) any = c.imp[(size_t)i * N2 + j] != 0;
            if (!any) continue;
            for (int j = 0; j < N2; ++j)
                if (c.imp[(size_t)i * N2 + j]) c.imp_cols[(size_t)j * c.imp_col_words + (k >> 6)] |= 1ull << (k & 63);
            ++k;
        }
    }
}

int load_code(const char* path, Code& c)
{
    std::ifstream ifs(path, std::ios::binary);
    if (!ifs.is_open()) return fail(QEC_ERR_IO, std::string("Unable to find code file ") + path);
    std::string params, hc, hd, imp;
    std::getline(ifs, params);
    std::getline(ifs, hc);
    std::getline(ifs, hd);
    std::getline(ifs, imp);
    std::istringstream ps(params);
    if (params.compare(0, 3, "css") == 0 && (params.size() == 3 || params[3] == ' ' || params[3] == '\t')) {
        // "css n mX mZ": a general code, the matrices in the same syntax
        ps.ignore(3);
        long n = 0, mX = 0, mZ = 0;
        if (!(ps >> n >> mX >> mZ))
            return fail(QEC_ERR_FORMAT, std::string("code file has no 'css n mX mZ' header: ") + path);
        if (n <= 0 || mX <= 0 || mZ <= 0 || n > (1 << 20) || mX > (1 << 20) || mZ > (1 << 20))
            return fail(QEC_ERR_FORMAT, "code file header out of range");
        // the dense matrices are allocated from the header: bound them as the six-number form bounds L P
        const long kMaxEntries = 1L << 28;
        if (mX * n > kMaxEntries || mZ * n > kMaxEntries)
            return fail(QEC_ERR_FORMAT, "code file header out of range (a matrix of more than 2^28 entries)");
        const bool has_imp = !imp.empty() && imp.find_first_not_of(" \t\r") != std::string::npos;
        if (has_imp && 4 * n * n > kMaxEntries)
            return fail(QEC_ERR_FORMAT, "code file: an I-P line of more than 2^28 entries (qec_code_with_logical derives the check)");
        std::vector<uint8_t> HX, HZ, IMP;
        parse_matrix(hc, HX, (size_t)mX * n);
        parse_matrix(hd, HZ, (size_t)mZ * n);
        if (has_imp) parse_matrix(imp, IMP, 4 * (size_t)n * n);
        return general_code((int)n, (int)mX, HX.data(), (int)mZ, HZ.data(), IMP.empty() ? nullptr : IMP.data(), c);
    }
    if (!(ps >> c.J >> c.K >> c.L >> c.P >> c.sigma >> c.tau))
        return fail(QEC_ERR_FORMAT, std::string("code file has no 'J K L P sigma tau' header: ") + path);
    if (c.J <= 0 || c.K <= 0 || c.L <= 0 || c.P <= 0 || (long)c.L * c.P > (1 << 20))
        return fail(QEC_ERR_FORMAT, "code file header out of range");
    const size_t n = (size_t)c.L * c.P;
    parse_matrix(hc, c.pcmX, (size_t)c.J * c.P * n);
    parse_matrix(hd, c.pcmZ, (size_t)c.K * c.P * n);
    if (!imp.empty()) parse_matrix(imp, c.imp, 4 * n * n);
    else c.imp.clear();
    finalize_code(c);
    return QEC_OK;
}

bool generator_exponents(int J, int K, int L, int P, int sigma, int tau, std::vector<int>& EX, std::vector<int>& EZ)
{
    // sigma^-1: the element of Z_P^* with x*sigma = 1 mod P (QEC_LDPC_CSS.cu:37-39)
    long inv = -1;
    for (long x = 1; x < P; ++x)
        if ((x * sigma) % P == 1) { inv = x; break; }
    if (inv < 0) return false;
    auto spow = [&](long p) { return p < 0 ? pow_mod(inv, -p, P) : pow_mod(sigma, p, P); };
    EX.assign((size_t)J * L, 0);
    EZ.assign((size_t)K * L, 0);
    // HC (QEC_LDPC_CSS.cu:43-65): sigma^(l-j) left half, -(tau sigma^(j-1+l)) right half
    for (int j = 0; j < J; ++j)
        for (int l = 0; l < L; ++l) {
            long t = (l < L / 2) ? spow(l - j) : P - (tau * spow(j - 1 + l)) % P;
            EX[(size_t)j * L + l] = (int)(t % P);
        }
    // HD (QEC_LDPC_CSS.cu:67-90): tau sigma^(l-k-1) left half, -(sigma^(k+l)) right half
    for (int k = 0; k < K; ++k)
        for (int l = 0; l < L; ++l) {
            long t = (l < L / 2) ? (tau * spow(l - k - 1)) % P : P - spow(k + l);
            EZ[(size_t)k * L + l] = (int)(((t % P) + P) % P);
        }
    return true;
}

int generate_code(int J, int K, int L, int P, int sigma, int tau, Code& c)
{
    if (J <= 0 || K <= 0 || L <= 0 || P <= 1 || (long)L * P > (1 << 20))
        return fail(QEC_ERR_ARG, "qec_code_generate: J, K, L must be > 0 and P > 1");
    std::vector<int> EX, EZ;
    if (!generator_exponents(J, K, L, P, sigma, tau, EX, EZ))
        return fail(QEC_ERR_ARG, "qec_code_generate: sigma has no inverse mod P");
    c.J = J; c.K = K; c.L = L; c.P = P; c.sigma = sigma; c.tau = tau;
    const int n = L * P;
    // expand to circulant permutation blocks: col = (E + row % P) % P + l P (QEC_LDPC_CSS.cu:99-131)
    auto expand = [&](const std::vector<int>& E, int R, std::vector<uint8_t>& pcm) {
        pcm.assign((size_t)R * P * n, 0);
        for (int row = 0; row < R * P; ++row)
            for (int l = 0; l < L; ++l)
                pcm[(size_t)row * n + (E[(size_t)(row / P) * L + l] + row % P) % P + l * P] = 1;
    };
    expand(EX, J, c.pcmX);
    expand(EZ, K, c.pcmZ);
    c.imp.clear();
    finalize_code(c);
    return QEC_OK;
}

namespace {
// m x n dense 0/1 matrix -> bit-packed rows of W = ceil(n / 64) words
std::vector<uint64_t> pack_rows(const std::vector<uint8_t>& H, int m, int n)
{
    const int W = (n + 63) / 64;
    std::vector<uint64_t> R((size_t)m * W, 0);
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < n; ++j)
            if (H[(size_t)i * n + j]) R[(size_t)i * W + (j >> 6)] |= 1ull << (j & 63);
    return R;
}

// A basis of ker(H) over GF(2), one n-bit row per free column in ascending order: H is reduced to
// reduced row-echelon form with pivots taken left to right; the row of free column f is e_f plus
// e_pivot(r) for every pivot row r with R[r][f] = 1.  v is in rowspace(H) iff every basis row has
// even overlap with v (rowspace(H) = ker(H)^perp).
std::vector<std::vector<uint64_t>> kernel_basis(const std::vector<uint8_t>& H, int m, int n)
{
    const int W = (n + 63) / 64;
    std::vector<uint64_t> R = pack_rows(H, m, n);
    std::vector<int> pivot_col;  // of pivot row r
    std::vector<uint8_t> is_pivot(n, 0);
    int rank = 0;
    for (int col = 0; col < n && rank < m; ++col) {
        const int w = col >> 6;
        const uint64_t bit = 1ull << (col & 63);
        int sel = -1;
        for (int i = rank; i < m; ++i)
            if (R[(size_t)i * W + w] & bit) { sel = i; break; }
        if (sel < 0) continue;
        if (sel != rank) std::swap_ranges(&R[(size_t)sel * W], &R[(size_t)sel * W] + W, &R[(size_t)rank * W]);
        const uint64_t* pr = &R[(size_t)rank * W];
        for (int i = 0; i < m; ++i)
            if (i != rank && (R[(size_t)i * W + w] & bit))
                for (int k = 0; k < W; ++k) R[(size_t)i * W + k] ^= pr[k];
        pivot_col.push_back(col);
        is_pivot[col] = 1;
        ++rank;
    }
    std::vector<std::vector<uint64_t>> basis;
    for (int f = 0; f < n; ++f) {
        if (is_pivot[f]) continue;
        std::vector<uint64_t> row(W, 0);
        row[f >> 6] |= 1ull << (f & 63);
        for (int r = 0; r < rank; ++r)
            if (R[(size_t)r * W + (f >> 6)] & (1ull << (f & 63))) row[pivot_col[r] >> 6] |= 1ull << (pivot_col[r] & 63);
        basis.push_back(std::move(row));
    }
    return basis;
}
}  // namespace

void code_degrees(const Code& c, int out[5])
{
    for (int sec = 0; sec < 2; ++sec) {
        const std::vector<uint8_t>& H = sec ? c.pcmZ : c.pcmX;
        const int m = sec ? c.mZ : c.mX, n = c.n;
        std::vector<int> col(n, 0);
        int rw = 0;
        for (int r = 0; r < m; ++r) {
            int w = 0;
            for (int v = 0; v < n; ++v)
                if (H[(size_t)r * n + v]) { ++w; ++col[v]; }
            rw = std::max(rw, w);
        }
        out[sec] = rw;
        out[2 + sec] = n ? *std::max_element(col.begin(), col.end()) : 0;
    }
    out[4] = std::max(out[0], out[1]);
}

// The layers of the serial schedule: the checks in ascending index, each with the smallest
// colour none of whose checks shares a variable with it.  used[l][v]: a check of colour l contains v.
int code_layers(const Code& c, int sector, int32_t* colour)
{
    const std::vector<uint8_t>& H = sector ? c.pcmZ : c.pcmX;
    const int m = sector ? c.mZ : c.mX, n = c.n;
    std::vector<std::vector<uint8_t>> used;
    std::vector<int> vars;
    for (int r = 0; r < m; ++r) {
        vars.clear();
        for (int v = 0; v < n; ++v)
            if (H[(size_t)r * n + v]) vars.push_back(v);
        size_t l = 0;
        for (; l < used.size(); ++l) {
            bool shared = false;
            for (int v : vars) shared |= used[l][v] != 0;
            if (!shared) break;
        }
        if (l == used.size()) used.emplace_back(n, 0);
        for (int v : vars) used[l][v] = 1;
        if (colour) colour[r] = (int32_t)l;
    }
    return (int)used.size();
}

void code_layer_order(const Code& c, int sector, std::vector<int32_t>& order, std::vector<int32_t>& offset)
{
    const int m = sector ? c.mZ : c.mX;
    std::vector<int32_t> colour(m);
    const int layers = code_layers(c, sector, colour.data());
    offset.assign(layers + 1, 0);
    for (int r = 0; r < m; ++r) ++offset[colour[r] + 1];
    for (int l = 0; l < layers; ++l) offset[l + 1] += offset[l];
    order.resize(m);
    std::vector<int32_t> next(offset.begin(), offset.end() - 1);
    for (int r = 0; r < m; ++r) order[next[colour[r]]++] = r;  // ascending index inside a colour
}

int general_code(int n, int mX, const uint8_t* HX, int mZ, const uint8_t* HZ, const uint8_t* imp, Code& c)
{
    if (n <= 0 || mX <= 0 || mZ <= 0)
        return fail(QEC_ERR_ARG, "qec_code_from_matrices: n, mX and mZ must be > 0");
    if (!HX || !HZ) return fail(QEC_ERR_ARG, "qec_code_from_matrices: null matrix");
    for (int sec = 0; sec < 2; ++sec) {
        const uint8_t* H = sec ? HZ : HX;
        const int m = sec ? mZ : mX;
        const char* name = sec ? "HZ" : "HX";
        for (int r = 0; r < m; ++r) {
            bool any = false;
            for (int v = 0; v < n; ++v) {
                const uint8_t x = H[(size_t)r * n + v];
                if (x > 1)
                    return fail(QEC_ERR_ARG, std::string("qec_code_from_matrices: ") + name + "[" + std::to_string(r) + "][" +
                                                 std::to_string(v) + "] = " + std::to_string((int)x) + " is not 0 or 1");
                any |= x != 0;
            }
            if (!any)
                return fail(QEC_ERR_ARG, std::string("qec_code_from_matrices: row ") + std::to_string(r) + " of " + name +
                                             " is all zero (a check on no qubit)");
        }
    }
    c = Code();
    c.general = true;
    c.n = n; c.mX = mX; c.mZ = mZ;
    c.pcmX.assign(HX, HX + (size_t)mX * n);
    c.pcmZ.assign(HZ, HZ + (size_t)mZ * n);
    if (imp) c.imp.assign(imp, imp + 4 * (size_t)n * n);
    int deg[5];
    code_degrees(c, deg);
    c.dvX = deg[2]; c.dvZ = deg[3]; c.D = deg[4];
    // k = n - rank HX - rank HZ: a kernel basis has n - rank rows
    c.k = (int)kernel_basis(c.pcmX, mX, n).size() + (int)kernel_basis(c.pcmZ, mZ, n).size() - n;
    finalize_code(c);
    return QEC_OK;
}

int derive_logical(const Code& src, int mode, Code& out)
{
    if (mode != QEC_LOGICAL_REFERENCE && mode != QEC_LOGICAL_DEGENERATE)
        return fail(QEC_ERR_ARG, "qec_code_with_logical: mode must be QEC_LOGICAL_REFERENCE or QEC_LOGICAL_DEGENERATE");
    const int n = src.n, N2 = 2 * n;
    if (N2 > 4096)
        return fail(QEC_ERR_UNSUPPORTED, "qec_code_with_logical: 2n > 4096 (the limit of the device statistics tables)");
    if (mode == QEC_LOGICAL_DEGENERATE) {
        // the rows of pcmZ (pcmX) are harmless x (z) residuals only if the two stabilizer sets commute
        const int W = (n + 63) / 64;
        const std::vector<uint64_t> X = pack_rows(src.pcmX, src.mX, n), Z = pack_rows(src.pcmZ, src.mZ, n);
        for (int i = 0; i < src.mX; ++i)
            for (int j = 0; j < src.mZ; ++j) {
                uint64_t acc = 0;
                for (int k = 0; k < W; ++k) acc ^= X[(size_t)i * W + k] & Z[(size_t)j * W + k];
                if (__builtin_popcountll(acc) & 1)
                    return fail(QEC_ERR_UNSUPPORTED, "qec_code_with_logical: the degenerate check needs pcmX pcmZ^T = 0, "
                                                     "but the X and Z checks of this code do not commute");
            }
    }
    out = src;
    out.logical_mode = mode;
    const bool ref = mode == QEC_LOGICAL_REFERENCE;
    const auto bx = ref ? kernel_basis(src.pcmX, src.mX, n) : kernel_basis(src.pcmZ, src.mZ, n);
    const auto bz = ref ? kernel_basis(src.pcmZ, src.mZ, n) : kernel_basis(src.pcmX, src.mX, n);
    // block-diagonal [A 0; 0 B]: the x-half basis in rows [0, ..) of the upper-left n x n block, the
    // z-half basis in rows [n, ..) of the lower-right one
    out.imp.assign((size_t)N2 * N2, 0);
    for (size_t r = 0; r < bx.size(); ++r)
        for (int j = 0; j < n; ++j)
            if (bx[r][j >> 6] >> (j & 63) & 1) out.imp[r * N2 + j] = 1;
    for (size_t r = 0; r < bz.size(); ++r)
        for (int j = 0; j < n; ++j)
            if (bz[r][j >> 6] >> (j & 63) & 1) out.imp[(n + r) * N2 + n + j] = 1;
    finalize_code(out);
    return QEC_OK;
}

void host_syndrome(const Code& c, int sector, const uint8_t* e, uint8_t* s)
{
    const int R = sector ? c.K : c.J, P = c.P, L = c.L, n = c.n;
    if (c.is_qc) {
        const std::vector<int>& E = sector ? c.EZ : c.EX;
        for (int r = 0; r < R; ++r)
            for (int i = 0; i < P; ++i) {
                int x = 0;
                for (int l = 0; l < L; ++l) x ^= e[l * P + (E[(size_t)r * L + l] + i) % P] & 1;
                s[r * P + i] = (uint8_t)x;
            }
    } else {
        const std::vector<uint8_t>& H = sector ? c.pcmZ : c.pcmX;
        const int m = sector ? c.mZ : c.mX;  // R P for a file code
        for (int eq = 0; eq < m; ++eq) {
            int x = 0;
            for (int v = 0; v < n; ++v) x += H[(size_t)eq * n + v] * (e[v] & 1);
            s[eq] = (uint8_t)(x % 2);
        }
    }
}

bool host_check_logical(const Code& c, const uint8_t* ex, const uint8_t* ez)
{
    const int W = c.imp_words, n = c.n;
    std::vector<uint64_t> v(W, 0);
    for (int j = 0; j < n; ++j) {
        if (ex[j] & 1) v[j >> 6] |= 1ull << (j & 63);
        if (ez[j] & 1) v[(n + j) >> 6] |= 1ull << ((n + j) & 63);
    }
    const size_t rows = W ? c.imp_rows.size() / W : 0;
    for (size_t r = 0; r < rows; ++r) {
        const uint64_t* row = &c.imp_rows[r * W];
        uint64_t acc = 0;
        for (int w = 0; w < W; ++w) acc ^= row[w] & v[w];
        if (__builtin_popcountll(acc) & 1) return true;
    }
    return false;
}

Mt19937::Mt19937(uint32_t seed)
{
    mt[0] = seed;
    for (int i = 1; i < 624; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
    idx = 624;
}

uint32_t Mt19937::next()
{
    if (idx >= 624) {
        for (int i = 0; i < 624; ++i) {
            const uint32_t y = (mt[i] & 0x80000000u) | (mt[(i + 1) % 624] & 0x7fffffffu);
            mt[i] = mt[(i + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        }
        idx = 0;
    }
    uint32_t y = mt[idx++];
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

// VS2015 _Rng_from_urng: rejection on [0, 2^32) so that r % N is unbiased.
uint32_t Mt19937::msvc_uniform(uint32_t N)
{
    for (;;) {
        const uint32_t r = next();
        if (r / N < 0xFFFFFFFFu / N || 0xFFFFFFFFu % N == N - 1) return r % N;
    }
}

}  // namespace qec
