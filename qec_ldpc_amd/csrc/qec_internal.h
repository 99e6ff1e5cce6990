// Internal declarations shared by the libqecldpc translation units.
// Not part of the public interface (that is include/qec_ldpc.h).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/qec_ldpc.h"

namespace qec {

// BpArgs::hardPaths bits (from QEC_OPT_HARD_PATHS / QEC_OPT_CYCLE_JUMP / QEC_OPT_NEAR_HARD_JUMP / QEC_OPT_NEAR_PROBE)
enum { QEC_HP_FORMS = 1, QEC_HP_CYCLE = 2, QEC_HP_PHASE = 4 /* launch the instrumented kernel */,
       QEC_HP_NEAR = 8 /* the near-hard jump (qec_near.h); only with QEC_HP_FORMS */,
       QEC_HP_NEAR_PROBE = 16 /* its division-free probe (QEC_OPT_NEAR_PROBE); only with QEC_HP_NEAR */ };
// dispatch-order method (schedule.hip, launch_schedule): the global counting sort, the one-launch
// chunk-local order or the global sort in one launch with a software grid barrier (both measured
// slower; experiments)
enum { QEC_ORDER_GLOBAL = 0, QEC_ORDER_LOCAL = 1, QEC_ORDER_ONE_LAUNCH = 2 };

// Thread-local last-error text behind qec_last_error().
void set_error(const std::string& msg);
int fail(int status, const std::string& msg);

// Quantum_LDPC_Code (QEC_LDPC/Quantum_LDPC_Code.h:7-150) in circulant form.
// The dense pcmX/pcmZ/iMinusP of the reference are kept for API parity; the
// decoder itself only needs the exponent tables (one shift per P x P block).
struct Code {
    int J = 0, K = 0, L = 0, P = 0, sigma = 0, tau = 0;
    int n = 0, mX = 0, mZ = 0;
    std::vector<uint8_t> pcmX, pcmZ;   // m x n dense, as read / generated
    std::vector<uint8_t> imp;          // 2n x 2n dense I-P (empty for generated codes without a derived check)
    int logical_mode = 0;              // QEC_LOGICAL_*: imp from the file (or none), or derived (derive_logical)
    bool is_qc = false;                // every block a circulant permutation matrix
    // A general code (general_code: two 0/1 matrices, any degrees): J = K = L = P = sigma = tau = 0 and the
    // sizes are the matrices'.  D is the slot stride of its message / q_final layout (the largest row weight of
    // both sectors), dvX / dvZ its largest column weights, k = n - rank HX - rank HZ.
    bool general = false;
    int D = 0, dvX = 0, dvZ = 0, k = 0;
    int stride() const { return general ? D : L; }                         // slots per check
    int col_stride(int sector) const { return general ? (sector ? dvZ : dvX) : (sector ? K : J); }
    std::vector<int> EX, EZ;           // J x L / K x L shifts in [0, P): row i -> col (E + i) mod P
    // Bit-packed I-P rows that are not all-zero (for CheckLogicalError).
    int imp_words = 0;                 // u64 words per packed 2n-bit row
    std::vector<uint64_t> imp_rows;    // nnz_rows x imp_words
    // Columns of I-P over its non-zero rows (2n x imp_col_words, bit k = k-th non-zero row): the
    // device statistics kernels XOR the columns at the residual's set bits.
    int imp_col_words = 0;
    std::vector<uint64_t> imp_cols;
    std::string describe() const;      // operator<< of Quantum_LDPC_Code.h:145-150
};

int load_code(const char* path, Code& out);
int generate_code(int J, int K, int L, int P, int sigma, int tau, Code& out);
// A general code from dense row-major 0/1 bytes (qec_code_from_matrices); imp (nullable) is a 2n x 2n I-P matrix.
int general_code(int n, int mX, const uint8_t* HX, int mZ, const uint8_t* HZ, const uint8_t* imp, Code& out);
// max row weight X, Z, max column weight X, Z, slot stride (qec_code_degrees); any code
void code_degrees(const Code& c, int out[5]);
// The serial schedule's layers of one sector (qec_code_layers): colour[m] (nullable); returns their number
int code_layers(const Code& c, int sector, int32_t* colour);
// The sector's processing order under the serial schedule: its checks sorted by (colour, index), and the first
// position of each layer in that order (layers + 1 entries, the last = m)
void code_layer_order(const Code& c, int sector, std::vector<int32_t>& order, std::vector<int32_t>& offset);
// Generator exponent tables (QEC_LDPC/QEC_LDPC_CSS.cu:37-90); returns false if sigma has no inverse.
bool generator_exponents(int J, int K, int L, int P, int sigma, int tau, std::vector<int>& EX, std::vector<int>& EZ);
void finalize_code(Code& c);  // derive circulant tables + packed I-P from the dense matrices
// A copy of src whose logical check is derived from its parity-check matrices (QEC_LOGICAL_REFERENCE:
// rx not in rowspace(pcmX) or rz not in rowspace(pcmZ), what the shipped I-P files compute;
// QEC_LOGICAL_DEGENERATE: rx not in rowspace(pcmZ) or rz not in rowspace(pcmX), needs pcmX pcmZ^T = 0):
// a block-diagonal imp whose rows are kernel bases of the two matrices.  2n <= 4096.
int derive_logical(const Code& src, int mode, Code& out);

// Host syndrome s = H e mod 2 via the circulant tables (or dense if not QC).
void host_syndrome(const Code& c, int sector, const uint8_t* e, uint8_t* s);
// CheckLogicalError (Quantum_LDPC_Code.h:126-142) on [ex | ez].
bool host_check_logical(const Code& c, const uint8_t* ex, const uint8_t* ez);

// std::mt19937 + VS2015 uniform_int_distribution, the
// stream the reference's published seeds were drawn from.
struct Mt19937 {
    uint32_t mt[624];
    int idx;
    explicit Mt19937(uint32_t seed);
    uint32_t next();
    uint32_t msvc_uniform(uint32_t N);  // uniform_int_distribution<int>(0, N-1)
};

// Host description of a fused Monte-Carlo front-end launch (montecarlo.hip,
// mc_errors_syndrome_kernel, or mc_gap_kernel for PHILOX): error source (MC_SRC_*), syndromes out,
// packed errors out.
enum { MC_SRC_PHILOX = 0, MC_SRC_DRAWS = 1, MC_SRC_BYTES = 2, MC_SRC_INDEPENDENT = 3 /* over the handle's priors */,
       MC_SRC_PAULI = 4 /* the handle's Pauli channel */ };
// the fused low-p Monte-Carlo pipeline's stages (triage.hip, launch_mc_fused)
enum { MC_FUSED_SAMPLE = 0, MC_FUSED_SURVIVORS = 1 };
struct McArgsHost {
    const Code* code = nullptr;
    uint64_t seed = 0, start = 0;
    float p = 0.0f;                 // PHILOX
    const int32_t* idx = nullptr;   // DRAWS
    const uint8_t* type = nullptr;
    int W = 0;
    const uint8_t* x = nullptr;     // BYTES
    const uint8_t* z = nullptr;
    const float* prior = nullptr;   // INDEPENDENT (with seed, start): device priors, sector X [n] then Z [n]
    const uint64_t* pauli_thr = nullptr;  // PAULI (with seed, start): device thresholds tX [n], tXY [n], tXYZ [n]
    uint8_t* sX = nullptr;
    uint8_t* sZ = nullptr;
    uint32_t* sXp = nullptr;        // PHILOX only: syndromes as bit rows [B][ceil(mX/32)] words instead
    uint32_t* sZp = nullptr;
    uint8_t* errp = nullptr;        // [B][2 ceil(n/8)], nullable
    bool errp_words = false;        // PHILOX only: errp rows padded to whole words (4 ceil(2 ceil(n/8) / 4) B)
    const int32_t* chkVar = nullptr;  // non-QC codes: check -> variables (BYTES, DRAWS)
    const int32_t* varEdge = nullptr; // non-QC codes: variable -> edges (PHILOX, the gap walk)
    long long B = 0;
};

// Scaled min-sum in the LLR domain (QEC_OPT_BP_METHOD = 1; DESIGN.md section 2, "The min-sum form"), both engines
constexpr uint32_t kMinSumCap = 0x49800000u;        // K: the pattern of 2^20, the cap of a check's magnitudes
constexpr float kMinSumLlrMax = 1073741824.0f;      // Lambda = 2^30: the clamp of a channel LLR
constexpr float kMinSumInside = 4.5951198f;         // ln 99: a message M is inside iff |M| < this
constexpr int kMinSumDefaultScale = 160;            // QEC_OPT_MINSUM_SCALE: alpha = k / 256
// The channel LLR of a prior (qec_minsum_llr; cpu_engine.cpp): one host function for both engines
float minsum_llr(float prior);

// One decode launch of the sparse-graph engine (bp_sparse.hip, launch_decode_sparse); every pointer is a device pointer.
struct SparseDecode {
    // the decode buffers and the arguments of Decode
    const uint8_t* sX = nullptr;
    const uint8_t* sZ = nullptr;
    long long B = 0;
    float errorProbability = 0.0f;
    int maxIter = 0;
    int stop = QEC_STOP_REF;
    uint8_t* eX = nullptr;
    uint8_t* eZ = nullptr;
    uint8_t* flags = nullptr;
    int32_t* iters = nullptr;       // nullable
    float* q = nullptr;             // nullable
    // the kernel variant and its tables
    const float* prior = nullptr;   // nullptr: the scalar kernels (errorProbability); else the 2n priors (PRIORS kernels)
    int corr = 0;                   // QEC_OPT_CORRELATED: 0, or 1 / 2 for the CORR kernels with first sector X / Z
    const float* cond = nullptr;    // CORR with prior set: the 4n conditional priors
    float c0 = 0.0f, c1 = 0.0f;     // CORR without prior: the scalar pair (correlated_priors)
    int serial = 0;                 // QEC_OPT_BP_SCHEDULE: 1 for the SERIAL kernels (scalar p' or prior; never with corr)
    // QEC_OPT_BP_METHOD = 1: 0, or the scale k (alpha = k / 256) for the MINSUM kernels (never with corr or serial);
    // they decode under lam = minsum_llr(p') or, with prior set, under llr = the 2n channel LLRs
    int minsum = 0;
    float lam = 0.0f;
    const float* llr = nullptr;
    // qec_decoder_set_relay (with minsum): the RELAY kernels under gamma = the tables [legs][sector][n], solutions = S and
    // relay_weight = nullptr (w_v = 1) or the 2n integer weights of the handle's priors; gamma = nullptr: plain min-sum
    const float* gamma = nullptr;
    int legs = 0, solutions = 0;
    const int32_t* relay_weight = nullptr;
    // QEC_OPT_MINSUM_SCHEDULE = 1 (with minsum, gamma = nullptr): the LAYERED kernels, layered min-sum
    int layered = 0;
    // qec_decoder_set_syndrome_priors (with minsum, gamma = nullptr): the SOFT kernels under mu = the mX + mZ channel LLRs
    // of the measurement-error variables; fX / fZ (nullable) receive the measurement decisions, [B][mX] and [B][mZ]
    const float* mu = nullptr;
    uint8_t* fX = nullptr;
    uint8_t* fZ = nullptr;
};

// The relay form: the limits of qec_decoder_set_relay
constexpr int kRelayMaxLegs = 1024;
constexpr long long kRelayMaxEntries = 1LL << 22;   // legs x n
constexpr int kRelayMaxSolutions = 64;

}  // namespace qec
