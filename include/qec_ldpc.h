/*
 * qec_ldpc.h -- C ABI of libqecldpc.so, the MI355X (gfx950) belief-propagation
 * decoder for quasi-cyclic CSS quantum LDPC codes.
 *
 * Plain C: opaque handles, plain pointers and sizes, int status codes
 * (0 = ok, < 0 = error, text in qec_last_error()).  No HIP or torch types
 * appear in any signature; streams are passed as `void*` (a hipStream_t or NULL).
 *
 * Each entry point names the reference interface it replaces
 * (cantwellc/QEC_LDPC, paths relative to the repository root).
 *
 * Threading: a qec_code is immutable after creation and may be shared.  Calls on
 * one qec_decoder are serialised by the caller (like one DecoderCPU per OpenMP
 * thread, QEC_LDPC/DecoderCPU.h:431); distinct decoders may be driven from
 * distinct host threads.
 *
 * Streams: the device-pointer (_dev) entry points enqueue on the caller's stream and
 * return without synchronising.  A decoder's workspace (dispatch order, flag-merge
 * words) is reused by every launch; a launch on a stream other than the previous
 * launch's first waits for that launch (an event), so calls on one decoder from
 * several streams are ordered, not concurrent.  For concurrency use one decoder per
 * stream.  Every entry point restores the caller's current HIP device.
 */
#ifndef QEC_LDPC_H
#define QEC_LDPC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QEC_LDPC_ABI_VERSION 4

/* status codes */
enum {
    QEC_OK = 0,
    QEC_ERR_ARG = -1,          /* bad argument (null pointer, out-of-range size) */
    QEC_ERR_IO = -2,           /* file missing/unreadable ("Unable to find code file", Quantum_LDPC_Code.h:78) */
    QEC_ERR_FORMAT = -3,       /* malformed code file */
    QEC_ERR_UNSUPPORTED = -4,  /* code shape the GPU engine does not handle */
    QEC_ERR_HIP = -5,          /* HIP runtime error / no GPU */
    QEC_ERR_NOMEM = -6
};

/* ErrorCode bit flags, identical to Decoder::ErrorCode (QEC_LDPC/Decoder.h:14-23) */
enum {
    QEC_SUCCESS = 0,
    QEC_SYNDROME_FAIL_X = 1 << 0,
    QEC_SYNDROME_FAIL_Z = 1 << 1,
    QEC_SYNDROME_FAIL_XZ = QEC_SYNDROME_FAIL_X | QEC_SYNDROME_FAIL_Z,
    QEC_CONVERGENCE_FAIL_X = 1 << 2,
    QEC_CONVERGENCE_FAIL_Z = 1 << 3,
    QEC_CONVERGENCE_FAIL_XZ = QEC_CONVERGENCE_FAIL_X | QEC_CONVERGENCE_FAIL_Z
};

/* BP stop rules */
enum {
    QEC_STOP_REF = 0,      /* DecoderCPU::BeliefPropogation (DecoderCPU.h:280-291): convergence test at n % 10 == 0 */
    QEC_STOP_FIXED = 1,    /* exactly maxIterations iterations (the headline "fixed BP iters") */
    QEC_STOP_SYNDROME = 2  /* stop once the hard decision satisfies the syndrome (per sector) */
};

enum { QEC_SECTOR_X = 0, QEC_SECTOR_Z = 1 };

/* GPU engines behind one decoder handle */
enum {
    QEC_ENGINE_AUTO = 0,       /* wave-circulant if the code has an instantiated kernel, else sparse-graph */
    QEC_ENGINE_CIRCULANT = 1,  /* wave-circulant: circulant-permutation QC codes, P <= 64 (bp_decode.hip) */
    QEC_ENGINE_SPARSE = 2,     /* sparse-graph: any code DecoderCPU accepts (regular, dc = L, dv = J / K) */
    QEC_ENGINE_CPU = 3         /* host threads, device -1 (DecoderCPU's drop-in; cpu_engine.cpp) */
};

typedef struct qec_code qec_code;
typedef struct qec_decoder qec_decoder;

/* CodeStatistics (QEC_LDPC/CodeStatistics.h:5-20) counters */
typedef struct {
    uint32_t randSeed;
    uint32_t numErrorsTested;
    uint32_t numXErrorsTested;
    uint32_t numZErrorsTested;
    uint32_t errorWeight;
    uint32_t corrected;
    uint32_t syndromeErrorsX;
    uint32_t syndromeErrorsZ;
    uint32_t logicalErrors;
    uint32_t convergenceFailX;
    uint32_t convergenceFailZ;
    int64_t durationMicroSeconds;
} qec_stats;

/* ---- diagnostics ---------------------------------------------------------- */
const char* qec_last_error(void);  /* message of the last failing call on this thread */
int qec_abi_version(void);         /* QEC_LDPC_ABI_VERSION */
/* Build id of this library: a hash of the sources and flags it was compiled from (the same for every
 * rebuild of the same tree); rocprofv3 profiles are stamped with it (tools/gpu/pmc_summary.py). */
const char* qec_build_id(void);

/* ---- code model ----------------------------------------------------------- */
/* Replaces Quantum_LDPC_Code::createFromFile (QEC_LDPC/Quantum_LDPC_Code.h:26-80):
 * 4-line text file "J K L P sigma tau" / HX / HZ / I-P.  NULL on error.
 * A first line "css n mX mZ" instead reads a general code (qec_code_from_matrices): HX (mX x n), HZ
 * (mZ x n) and an optional I-P line (2n x 2n) follow in the same matrix syntax. */
qec_code* qec_code_load(const char* path);
/* A general CSS code from its two parity-check matrices (no reference analogue), dense row-major 0/1
 * bytes HX: mX x n, HZ: mZ x n.  Any row and column weights; an all-zero column (a qubit in no check of
 * that sector) is allowed.  The code has J = K = L = P = sigma = tau = 0, no I-P matrix
 * (qec_code_with_logical derives one) and no exponent tables.  Its message / q_final layout has one
 * slot stride D for both sectors, the largest row weight (qec_code_degrees); BP runs each node with its
 * own degree.  The sparse-graph engine and the CPU engine decode it (D <= 32 and
 * column weights <= 16 on the GPU).  NULL with QEC_ERR_ARG for an entry other than 0 / 1, an all-zero
 * row, or n, mX or mZ <= 0; the text names the row or entry. */
qec_code* qec_code_from_matrices(int n, int mX, const uint8_t* HX, int mZ, const uint8_t* HZ);
/* out[5] = largest row weight of HX, of HZ, largest column weight of HX, of HZ, and the slot stride
 * D = the larger row weight.  Any code; a regular one gives L, L, J, K, L. */
int qec_code_degrees(const qec_code* code, int* out5);
/* The layers of the serial BP schedule (QEC_OPT_BP_SCHEDULE) for one sector: walking the sector's checks in
 * ascending index, check c gets the smallest colour l >= 0 such that no check already coloured l shares a
 * variable with c.  colour: numEqs entries, nullable.  Returns the number of layers (< 0 on error).  Checks of
 * one colour share no variable; a circulant-permutation QC code gives colour c / P. */
int qec_code_layers(const qec_code* code, int sector, int32_t* colour);
/* 1 if the code has wave min-sum kernels (QEC_OPT_MINSUM_WAVE): a circulant-permutation code with 1 <= P <= 64 whose
 * block shape (J, K, L) is one of (4,5,10) (3,3,6) (2,3,6) (3,4,8) (4,4,8) (3,5,10) (4,6,12) (2,2,4); else 0.  A host
 * query: no device is touched.  (< 0 on error.) */
int qec_code_has_wave_minsum(const qec_code* code);
/* Replaces the QC_LDPC_CSS(J,K,L,P,sigma,tau) generator (QEC_LDPC/QEC_LDPC_CSS.cu:5-131).
 * Generated codes carry no I-P matrix (the reference never generates one); qec_code_with_logical
 * derives the check from the two matrices. */
qec_code* qec_code_generate(int J, int K, int L, int P, int sigma, int tau);
int qec_code_free(qec_code* code);
/* J K L P sigma tau n numEqsX numEqsZ (Quantum_LDPC_Code.h:10-20) into out[9] */
int qec_code_params(const qec_code* code, int* out9);
/* circulant shift of every P x P block, J x L (X) or K x L (Z), row-major;
 * returns QEC_ERR_UNSUPPORTED if the code is not a circulant-permutation QC code */
int qec_code_exponents(const qec_code* code, int sector, int* out);
/* dense parity-check matrix pcmX / pcmZ (m x n, 0/1) */
int qec_code_pcm(const qec_code* code, int sector, uint8_t* out);
/* "[J=..,K=..,L=..,P=..,s=..,t=..][[n=..,k=..]]" (Quantum_LDPC_Code.h:145-150); a general code:
 * "[[n=..,k=..]]" with k = n - rank HX - rank HZ */
int qec_code_describe(const qec_code* code, char* buf, size_t len);
/* Quantum_LDPC_Code::GetSyndromeX/Z (Quantum_LDPC_Code.h:94-124) for B error vectors,
 * e: B x n (0/1) -> s: B x m (host memory) */
int qec_code_syndrome(const qec_code* code, int sector, const uint8_t* e, size_t B, uint8_t* s);
/* Quantum_LDPC_Code::CheckLogicalError (Quantum_LDPC_Code.h:126-142) on the
 * residual [ex | ez] of B samples; out[b] = 1 if logical error */
int qec_code_check_logical(const qec_code* code, const uint8_t* ex, const uint8_t* ez, size_t B, uint8_t* out);
/* The logical check derived from the two parity-check matrices (no reference analogue: the reference
 * reads the I-P matrix from line 4 of a code file and never generates one).
 *   QEC_LOGICAL_FILE: the matrix of the code file, if it had one.
 *   QEC_LOGICAL_REFERENCE: logical iff rx is not in rowspace(pcmX) or rz is not in rowspace(pcmZ).
 *     This is what the shipped I-P matrices compute: they are block-diagonal [A 0; 0 B] with
 *     ker A = rowspace(pcmX), ker B = rowspace(pcmZ).  On the residuals
 *     GetStatistics tests (rx in ker pcmX) nearly every non-zero residual is then a logical error,
 *     degenerate corrections included; the published counters carry that meaning.
 *   QEC_LOGICAL_DEGENERATE: logical iff rx is not in rowspace(pcmZ) or rz is not in rowspace(pcmX),
 *     so a residual that is a product of stabilizers counts as corrected.  Needs pcmX pcmZ^T = 0
 *     over GF(2) (otherwise NULL, QEC_ERR_UNSUPPORTED, "... do not commute").
 * The derived matrix is block-diagonal, its rows bases of ker(H) for the two matrices (reduced
 * row-echelon form, pivots left to right; one row per free column, ascending); every entry point
 * that takes a code with an I-P matrix takes it.  2n <= 4096 (QEC_ERR_UNSUPPORTED above). */
enum { QEC_LOGICAL_FILE = 0, QEC_LOGICAL_REFERENCE = 1, QEC_LOGICAL_DEGENERATE = 2 };
/* A NEW code with the same matrices and the derived check; `code` is untouched (a qec_code stays
 * immutable).  mode: QEC_LOGICAL_REFERENCE or QEC_LOGICAL_DEGENERATE.  NULL on error. */
qec_code* qec_code_with_logical(const qec_code* code, int mode);
int qec_code_logical_mode(const qec_code* code);            /* 0: the file's matrix, or none */
int qec_code_logical_rows(const qec_code* code, int* rows); /* non-zero rows of the check; 0 if none */
int qec_code_imp(const qec_code* code, uint8_t* out);       /* dense 2n x 2n; QEC_ERR_UNSUPPORTED if none */

/* ---- decoder (DecoderGPU, QEC_LDPC/DecoderGPU.h:11-281) ------------------- */
/* Replaces DecoderGPU(Quantum_LDPC_Code) (DecoderGPU.h:117-130) and, with device = -1,
 * DecoderCPU(Quantum_LDPC_Code) (DecoderCPU.h:16-39): the CPU engine, host threads over
 * edge-major tables, bit-identical decisions; it serves the host-buffer entry points and
 * qec_get_statistics (the _dev entry points and qec_monte_carlo need a GPU and fail with
 * QEC_ERR_UNSUPPORTED).  device >= 0 = HIP device ordinal.  max_batch sizes the
 * device-pointer workspace up front: the _dev decode entry points then allocate nothing
 * for B <= max_batch and may be captured into a graph.  Larger batches grow it on
 * demand (an error while the stream is being captured). */
qec_decoder* qec_decoder_create(const qec_code* code, int device, size_t max_batch);
/* Same with an explicit engine (QEC_ENGINE_*).  QEC_ENGINE_CIRCULANT fails with
 * QEC_ERR_UNSUPPORTED when the code has no wave-circulant kernel; QEC_ENGINE_SPARSE fails
 * for an irregular code (DecoderCPU's index tables assume row weight L and column weight
 * J / K, DecoderCPU.h:41-84). */
qec_decoder* qec_decoder_create_engine(const qec_code* code, int device, size_t max_batch, int engine);
int qec_decoder_destroy(qec_decoder* dec);
/* A decoder over several devices (the reference's sample-parallel loop, DecoderCPU.h:419-438,
 * spread over GPUs; main.cu:79,101 unchanged): one single-device part per entry of devices[]
 * (a device may appear more than once: two parts then share it).  The host-pointer entry
 * points (qec_decode_batch, qec_decode_batch_packed) split the batch into contiguous shards,
 * one per part, decoded concurrently; qec_get_statistics and qec_monte_carlo shard their
 * samples the same way and sum the parts' counters (bit-identical to one device: the counters
 * do not depend on sample order).  Options apply to every part.  The _dev entry points need
 * a single-device handle: call them on qec_decoder_part(dec, k).  Every ordinal must be >= 0
 * (QEC_ERR_ARG otherwise: a group is GPU-only). */
qec_decoder* qec_decoder_create_multi(const qec_code* code, const int* devices, int ndevices, size_t max_batch);
/* The same with every part created by qec_decoder_create_engine(.., engine): QEC_ENGINE_AUTO (as above),
 * QEC_ENGINE_CIRCULANT or QEC_ENGINE_SPARSE (QEC_ENGINE_CPU: QEC_ERR_ARG). */
qec_decoder* qec_decoder_create_multi_engine(const qec_code* code, const int* devices, int ndevices, size_t max_batch,
                                             int engine);
int qec_decoder_num_parts(const qec_decoder* dec);      /* 1 for a single-device decoder */
qec_decoder* qec_decoder_part(qec_decoder* dec, int k); /* part k (the handle itself for k = 0 of a single one) */
int qec_decoder_device(const qec_decoder* dec);         /* HIP device ordinal (of part 0 for a group) */
/* Decoder options (no reference analogue: DecoderCPU has none).
 *   QEC_OPT_HARD_PATHS (default 1): once every message of a sector is exactly +0 or 1.0 the
 *     wave-circulant kernels switch to the exact hard-message forms of the check and variable
 *     updates (bp_decode.hip, check_pass_hard / var_pass).  Outputs are bit-identical either
 *     way; 0 forces the full arithmetic every iteration (for measurement).
 *   QEC_OPT_CYCLE_JUMP (default 1; needs QEC_OPT_HARD_PATHS): once a hard sector whose
 *     variables all carry equal messages takes an iteration that leaves every variable's inputs
 *     unchanged, the remaining iterations provably alternate between the two states just seen
 *     (bp_decode.hip, cycle_end), so the kernel jumps to the sector's last iteration.
 *     Bit-identical either way; 0 runs the remaining hard iterations one by one (for
 *     measurement).
 *   QEC_OPT_NEAR_HARD_JUMP (default 1; needs QEC_OPT_HARD_PATHS; fixed and reference stop, no q_final
 *     requested; wave-circulant kernels and the CPU engine): once a sector's messages are all within
 *     eps0 of 0 or 1, each variable's on one side, and those sides satisfy the syndrome, every later
 *     state provably stays so (eps0 per launch and sector from
 *     qec_near_hard_threshold), so the decisions, both flags and the iteration count are known and the
 *     sector jumps to its end.  Every output bit identical either way; 0 runs those iterations (for
 *     measurement).  A call that requests q_final, and the soft decode of the OSD stage, never jump.
 *     Nor does any decode of a general code (qec_code_from_matrices): the lemma is stated for one
 *     column weight R and one row weight L; outputs do not depend on the jump either way.
 *   QEC_OPT_SCHEDULE (default 1): dispatch order of the wave-circulant launch.  Two small
 *     kernels (a counting sort) order the batch by syndrome weight and the decode waves take syndromes heaviest
 *     first, so the rare syndromes that run every iteration in full arithmetic start early
 *     instead of extending the launch (schedule.hip); a sector-split launch orders each sector's
 *     waves by that sector's weight.  Outputs are written at each syndrome's
 *     own index and are bit-identical either way.  0 = batch order, 1 = sorted when
 *     4096 <= B <= 2^22 (codes with one syndrome per wave, P > 32: 4096 <= B <= 2^19, above which
 *     the pass costs more than it saves), 2 = sorted when B <= 2^22, 3 = as 2 but with the one-launch
 *     local order for B <= 2^18 short-row codes (each chunk sorted in LDS, chunks interleaved by rank;
 *     measured slower than the global sort at P7 65 536, kept for experiments), 4 = as 2 but the
 *     global sort in one launch with a software grid barrier for up to 128 chunks (measured slower).
 *     The workspace (10 B per syndrome + 1 MiB) is allocated
 *     by qec_decoder_create for max_batch and grown on demand by larger calls.
 *   QEC_OPT_SECTOR_SPLIT (default 1): the X and Z sectors of a syndrome are decoded by two
 *     waves instead of one after the other (halves the longest wave).  The launch then zeroes
 *     flags[] first and each sector ORs in its bits.  Bit-identical either way.  0 = off,
 *     1 = the kernel variant's measured choice (P7: split waves up to 2^20 syndromes, above 2^19 only
 *     with the per-sector dispatch order; P61: sector launches from 2^18 on under the fixed stop, at 2^20
 *     under the reference stop, at 2^20 and p >= 0.03 under the syndrome stop), 2 = on where the variant
 *     has split kernels (the two shipped codes),
 *     3 = sector launches: two launches on the caller's stream, sector X then
 *     sector Z, each kernel compiled (and its registers allocated) for its own sector only; the Z
 *     launch ORs its flags into the byte the X launch stored (shipped codes; elsewhere as 0).
 *   QEC_OPT_PHASE_STATS (default 0; measurement only, shipped codes): launches an instrumented
 *     copy of the kernel whose iters[] output packs, per sector, the iterations executed in each
 *     phase instead of their count: soft | hard << 8 | agreed << 16 | jumped << 24 (soft: full
 *     arithmetic; hard: hard-message forms; agreed: the agreement path; jumped: skipped by the
 *     cycle jump; each field mod 256).  Decisions and flags are unchanged.
 *   QEC_OPT_TRIAGE (default 1; shipped codes, syndrome stop with N >= 2 on the Monte-Carlo
 *     pipeline's bit-row syndromes, i.e. qec_monte_carlo): a triage kernel decides iteration 0 of
 *     64 syndromes per wave from the syndrome patterns (triage.hip); the sectors it does not stop
 *     are compacted into lists the decode kernel then decodes (list mode).  Bit-identical either
 *     way.  0 = off (every sector in the decode kernel), 1 = when p <= 0.01 (above it most
 *     sectors go on and the ordered decode of the whole batch is faster), 2 = always, 3 = as 1
 *     without the fused form.  Fused form (1, 2; depolarising qec_monte_carlo runs): sampler,
 *     syndromes, triage and the finished samples' statistics in one kernel, so only the samples
 *     with a sector that goes on reach HBM (list-mode decode, then their statistics).
 *   QEC_OPT_LAST_PATH (read only; qec_decoder_set_option refuses it): the launch sequence the
 *     handle's last decode call enqueued, as QEC_PATH_* bits (0 before the first decode), so a test
 *     can assert which kernels its comparison went through.
 *   QEC_OPT_MC_DECODE_TIME (default 1): qec_monte_carlo times its decode kernels with an event pair
 *     per batch (qec_mc_result.decodeSeconds).  0: no events between its launches (each costs the
 *     GPU a few microseconds, ~5 % of a 2^20-sample batch at p = 0.001) and decodeSeconds = 0;
 *     counters unchanged.
 *   QEC_OPT_OSD (default 0): BP + OSD-0.  0 = off (nothing changes); 1 = ordered-statistics decoding of
 *     order 0 as a post-processing stage of the SYNCHRONOUS calls (qec_decode_batch,
 *     qec_decode_batch_packed, qec_get_statistics, qec_monte_carlo); other values QEC_ERR_ARG.  For every
 *     sector whose SYNDROME_FAIL bit the main decode left set: the syndrome pair is decoded again with
 *     QEC_STOP_FIXED, the same errorProbability and QEC_OPT_OSD_ITERATIONS iterations; the columns of
 *     the sector's matrix are ordered by the final message r(v) at the lowest-index check that contains
 *     v (key: the bit pattern of r(v) with the sign bit cleared, 0x3F000000 for a NaN, compared as
 *     unsigned integers, descending, ties by v ascending); walking that order, a column becomes a pivot
 *     if it is linearly independent (GF(2)) of the pivots so far, up to rank(H); if [H | s] is consistent
 *     the estimate becomes the unique e supported on the pivots with H e = s and the sector's
 *     SYNDROME_FAIL bit is cleared, otherwise estimate and flag stay as BP left them (a syndrome entry
 *     other than 0 or 1 counts as inconsistent).  The other sector, the CONVERGENCE_FAIL bits and iters
 *     are untouched.  The result depends only on (code, syndrome, p, QEC_OPT_OSD_ITERATIONS), not on the
 *     engine, the batch or the main decode's path.  qec_monte_carlo then takes the unfused pipeline
 *     (sample, packed decode, OSD stage, statistics) and reads the number of failed samples back once
 *     per batch (one host synchronisation per batch); its counters describe the repaired estimates.
 *     The asynchronous _dev decode entry points IGNORE this option (their no-synchronisation,
 *     no-allocation contract stands): compose them with qec_osd_dev.  Limits of the kernel: n and the
 *     checks per sector <= 2048 and the bit-packed [H | s] within one workgroup's 64 KiB of LDS
 *     (QEC_ERR_UNSUPPORTED otherwise; the CPU engine has no limit).
 *   QEC_OPT_OSD_ITERATIONS (default 3, >= 1): iterations of the soft decode that orders the columns
 *     (a few: by the iteration cap a failing sector's fp32 posteriors are saturated and order nothing).
 *   QEC_OPT_OSD_SECTORS (read only): sectors the OSD stage repaired in the handle's last synchronous
 *     call (saturating; summed over the parts of a group).
 *   QEC_OPT_OSD_SWEEP (default 0; measurement only, GPU engines): how the OSD kernel XORs a pivot row
 *     into the rows that have the column's bit, per chunk of 64 rows.  1 = lanes across the row's words,
 *     one row after the other; 2 = each lane walks its own row; 0 = whichever takes fewer steps for the
 *     chunk (osd.hip).  Bit-identical in every state.
 *   QEC_OPT_OSD_ORDER (default 0, range 0 .. 64; other values QEC_ERR_ARG): lambda of the combination
 *     sweep (OSD-CS), with effect wherever the OSD stage runs (the synchronous calls under
 *     QEC_OPT_OSD = 1, qec_osd, qec_osd_dev).  With T = the non-pivot columns in the order of the walk
 *     (f = n - rank(H) of them), the candidates are, in this index order, the OSD-0 estimate, the f
 *     estimates with one column of T flipped, and those with two of the first min(lambda, f) columns of T
 *     flipped ({t_i, t_j}, i < j, by i then j); each is completed on the pivots so that H e = s.  The
 *     candidate of least Hamming weight becomes the estimate, among equals the lowest index.  0 = OSD-0
 *     exactly.  The result depends only on (code, syndrome, p, QEC_OPT_OSD_ITERATIONS, lambda).  A group
 *     applies the value to every part.  On a GPU handle lambda > 0 needs up to 65 more bit vectors over
 *     the checks in LDS: QEC_ERR_UNSUPPORTED if the sum passes one workgroup's 64 KiB.
 *   QEC_OPT_OSD_CS_SECTORS (read only): of the sectors counted by QEC_OPT_OSD_SECTORS, those whose
 *     lightest candidate was not the OSD-0 estimate (index > 0), in the handle's last synchronous call
 *     (saturating; summed over the parts of a group; zeroed and collected where QEC_OPT_OSD_SECTORS is).
 *   QEC_OPT_OSD_SCORE (default 0; 0 or 1, other values QEC_ERR_ARG): how the combination sweep scores its
 *     candidates.  0 = Hamming weight, as above.  1 = on a handle with priors
 *     (qec_decoder_set_priors) the sum, over the qubits a candidate flips, of that qubit's integer weight
 *     w(pi) = 0 for pi >= 1/2, 4095 for pi = 0, else min(4095, llrint(16 log2((1 - pi) / pi))) (sixteenths
 *     of a bit of log-likelihood ratio, the float pi taken exactly to double; one table per sector, built by
 *     qec_decoder_set_priors, read back with qec_decoder_get_osd_weights).  The least score wins, among
 *     equals the lowest candidate index; candidates, their order, the column order, the pivots, the flags
 *     and both counters are as under 0 (QEC_OPT_OSD_CS_SECTORS still counts winners of index > 0).  With
 *     effect wherever the OSD stage runs with lambda > 0 (the synchronous calls under QEC_OPT_OSD = 1,
 *     qec_osd, qec_osd_dev, which reads it at the call as it reads QEC_OPT_OSD_ORDER); at lambda = 0 there
 *     is one candidate and the order-0 kernel runs.  On a handle WITHOUT priors the value has no effect:
 *     every weight would be equal, score = w |e|, so the Hamming kernel runs and the winner is the same.
 *     The wave-circulant engine cannot hold priors and so never runs the weighted kernel.  A group applies
 *     the value (and the tables) to every part.  On a GPU handle the weighted sweep keeps 12 more bit
 *     vectors over the checks and one 16-bit weight per check in LDS: where a code fits at lambda under
 *     the Hamming score but not with these, the call that would make the weighted sweep run (this option,
 *     QEC_OPT_OSD_ORDER or qec_decoder_set_priors, whichever comes last) returns QEC_ERR_UNSUPPORTED and
 *     the text says so.  The result depends only on (code, syndrome, priors, QEC_OPT_OSD_ITERATIONS,
 *     lambda, this rule).
 *   QEC_OPT_CORRELATED (default 0; 0, 1 or 2, other values QEC_ERR_ARG): the correlated form of DESIGN.md
 *     section 2.  A Y error sets both bits of a qubit, so one sector's estimate says something about the other's
 *     bits.  0 = both sectors under their marginal priors, independently, as ever (the same kernels).  1 = the
 *     first sector F = X, the second S = Z; 2 = F = Z, S = X.  F is decoded exactly as under 0 (its estimate,
 *     its two flag bits, its iters entry and its block of q_final are the option-0 call's bit for bit); with
 *     d = F's final estimate (the bytes of eX / eZ), S is decoded by the prior form with
 *     pi_v = d[v] ? c1_S[v] : c0_S[v], its own iteration counter, last iteration and stop tests.  The tables:
 *     without priors c1 = 0.5f and c0 = (p / 3.0f) / (1.0f - 2.0f / 3.0f * p) in fp32 for both directions
 *     (qec_correlated_priors); with qec_decoder_set_priors alone c0_S = c1_S = S's marginal prior (independent
 *     marginals carry no correlation: every output bit equals the option-0 call); with a Pauli channel
 *     (qec_decoder_set_pauli_channel) its four conditional tables.  Sparse-graph engine (the CORR kernels of
 *     bp_sparse.hip; the plan, the workspace and the describe string are unchanged) and CPU engine (whose
 *     near-hard jump may fire for F and never fires for S); a wave-circulant handle refuses 1 and 2 with
 *     QEC_ERR_UNSUPPORTED and the text says to create the decoder with QEC_ENGINE_SPARSE.  Every decode entry
 *     point honours it, the _dev ones read it at the call (a captured graph keeps the kernels it captured), the
 *     OSD stage's soft decode goes through the same path; QEC_OPT_OSD_SCORE = 1 keeps scoring with the marginal
 *     tables and S is not decoded again after OSD repairs F.  A group applies the value to every part.
 *   QEC_OPT_BP_SCHEDULE (default 0; 0 or 1, other values QEC_ERR_ARG): the order of BP's updates (not the dispatch
 *     order of QEC_OPT_SCHEDULE).  0 = flooding, all checks and then all variables, as ever (the same kernels).
 *     1 = the serial (layered, check-sequential) schedule of DESIGN.md section 2: the state is one check->variable
 *     message R per real edge, 0.5f at the start (an unused slot of a general code +0.0f throughout).  An
 *     iteration takes the sector's checks in the order of qec_code_layers, sorted by (colour, index); check c
 *     forms, for each of its slots in ascending order, the message of the slot's variable v from pi_v and the R of
 *     v's OTHER checks as they stand (two running products from 1.0f - pi_v and pi_v in ascending check order,
 *     then P1 / (P0 + P1); pi_v = the prior of v, or p' = 2.0f / 3.0f * p), and then its own R by the check update
 *     of the flooding schedule.  The posterior of v is the same form over ALL its checks; its decision is
 *     posterior >= 0.5f; a variable in no check decides 0 and enters no test.  Stop rules over the posteriors:
 *     FIXED N iterations; SYNDROME after the first iteration whose decisions satisfy the syndrome; REF after an
 *     iteration with index % 10 == 0 that leaves no posterior inside (0.01, 0.99).  There is no special last
 *     iteration.  CONVERGENCE_FAIL: a posterior of the final state inside (0.01, 0.99); SYNDROME_FAIL from the
 *     final decisions; q_final: every real slot of v holds v's final posterior; N = 0 gives the posterior of the
 *     initial state.  Sparse-graph engine (the SERIAL kernels of bp_sparse.hip; plan, workspace, grid and describe
 *     string unchanged; the layer tables are uploaded when the plan is created, so setting the option allocates
 *     nothing) and CPU engine; a wave-circulant handle refuses 1 with QEC_ERR_UNSUPPORTED and the text says to
 *     create the decoder with QEC_ENGINE_SPARSE.  1 together with QEC_OPT_CORRELATED != 0 is refused with
 *     QEC_ERR_UNSUPPORTED by whichever qec_decoder_set_option comes second (the handle stays as it was).  Every
 *     decode entry point honours it, the _dev ones read it at the call (a captured graph keeps the kernels it
 *     captured); the OSD stage's soft decode runs the same schedule, so the stage's result then also depends on
 *     the schedule (its column key reads q_final, here the posterior).  The near-hard jump never fires under 1.
 *     A group applies the value to every part.
 *   QEC_OPT_BP_METHOD (default 0; 0 or 1, other values QEC_ERR_ARG): BP's message rule.  0 = the reference's fp32
 *     probability-domain product rule, as ever (the same kernels).  1 = scaled min-sum in the LLR domain, flooding
 *     ("The min-sum form"; LLR > 0 means the bit is 0).  The state is one fp32 LLR per real edge,
 *     at the start the channel LLR lambda_v of the edge's variable: qec_minsum_llr of v's prior, or of
 *     p' = 2.0f / 3.0f * p.  Check update: with a_k = bits(m_k) & 0x7FFFFFFF and g_k = bit 31 of input m_k, slot i
 *     gets the magnitude alpha * float_of(min as unsigned integers of 0x49800000 (= 2^20) and every a_k, k != i) and
 *     the sign t XOR the g_k of k != i, t = 1 iff the syndrome entry is non-zero.  Variable update: slot j gets the
 *     left fold lambda_v + r_0 + r_1 + ... without r_j, in ascending check order; the posterior is the fold over all
 *     r and the decision is posterior < 0.0f; in iteration N - 1 every slot of v gets the posterior.  A message M is
 *     inside iff fabsf(M) < 4.5951198f (ln 99).  Stop rules: FIXED N iterations; SYNDROME after the first iteration
 *     whose decisions satisfy the syndrome; REF at index % 10 == 0 when no real slot is inside.  CONVERGENCE_FAIL: a
 *     real slot of the final state inside; SYNDROME_FAIL and the estimate from the decisions of the last executed
 *     variable pass (N = 0: lambda_v < 0.0f); a variable in no check decides 0.  q_final holds the final slots as
 *     LLRs (an unused slot of a general code +0.0f); every value is finite.  Sparse-graph engine (the MINSUM kernels
 *     of bp_sparse.hip; plan, workspace, grid and describe string unchanged) and CPU engine; a wave-circulant handle
 *     refuses 1 with QEC_ERR_UNSUPPORTED and the text says to create the decoder with QEC_ENGINE_SPARSE.  1 together
 *     with QEC_OPT_CORRELATED != 0 or QEC_OPT_BP_SCHEDULE = 1 is refused with QEC_ERR_UNSUPPORTED by whichever
 *     qec_decoder_set_option comes second (the handle stays as it was).  Every decode entry point honours it, the
 *     _dev ones read it at the call and allocate nothing; the OSD stage's soft decode is min-sum too, and the stage,
 *     qec_osd and qec_osd_dev then order the columns by LLR ascending (q_final is an LLR).  The near-hard jump never
 *     fires under 1.  A group applies the value to every part.
 *   QEC_OPT_MINSUM_SCALE (default 160; 1 .. 256, other values QEC_ERR_ARG): the factor of min-sum's check update,
 *     alpha = (float)value / 256.0f (exact in fp32; the default is 0.625).  Read at the call, as the method is.
 *   QEC_OPT_MINSUM_WAVE (default 0; 0 or 1, other values QEC_ERR_ARG): a kernel choice of a sparse-engine handle.
 *     1 = the handle's plain min-sum decodes run the register-resident wave kernels (bp_wave_minsum.hip; DESIGN.md
 *     section 2, "The min-sum form in the wave layout"): one wave per G = 64 / P syndrome pairs, a sector's messages
 *     in registers, the same rule in the same evaluation order, so every output (estimates, flags, iteration
 *     counts, q_final) is the MINSUM kernels' bit for bit, with the scalar p or with the handle's priors.  The value
 *     is data, like QEC_OPT_MINSUM_SCALE: it takes effect in every decode while QEC_OPT_BP_METHOD = 1 and no relay
 *     tables are set; under the product rule it does nothing, and with relay tables the RELAY kernels run as before.
 *     QEC_PATH_WAVE is set in QEC_OPT_LAST_PATH exactly when the wave kernels ran.  The _dev entry points read it at
 *     the call and allocate nothing.  1 is refused with QEC_ERR_UNSUPPORTED (the handle stays as it was, the text
 *     names the reason) on a sparse handle whose code has no wave min-sum kernel (qec_code_has_wave_minsum), on a
 *     wave-circulant handle and on a CPU handle.  A group applies the value to every part.
 *   QEC_OPT_RELAY_WAVE (default 0; 0 or 1, other values QEC_ERR_ARG): a kernel choice of a sparse-engine handle,
 *     independent of QEC_OPT_MINSUM_WAVE.  1 = the handle's relay decodes (qec_decoder_set_relay) run the
 *     register-resident wave kernels (bp_wave_relay.hip; DESIGN.md section 2, "The relay form in the wave layout"):
 *     one wave per G = 64 / P syndrome pairs, a sector's messages, memories and best solution in registers, each
 *     group of the wave in a leg of its own, the same rule in the same evaluation order, so every output (estimates,
 *     flags, iteration counts, q_final) is the RELAY kernels' bit for bit, with the scalar p or with the handle's
 *     priors.  The value is data: it takes effect in every decode while QEC_OPT_BP_METHOD = 1 and relay tables are
 *     set; without tables or under the product rule it does nothing (plain min-sum follows QEC_OPT_MINSUM_WAVE, and so
 *     does the OSD stage's soft decode).  QEC_PATH_WAVE is then set beside QEC_PATH_RELAY in QEC_OPT_LAST_PATH; with
 *     the option at 0 a relay decode never sets it.  The _dev entry points read it at the call and allocate nothing.
 *     1 is refused with QEC_ERR_UNSUPPORTED (the handle stays as it was, the text names the reason) on a sparse
 *     handle whose code has no wave kernel (qec_code_has_wave_minsum answers for both options), on a wave-circulant
 *     handle and on a CPU handle.  A group applies the value to every part.
 *   QEC_OPT_MINSUM_SCHEDULE (default 0; 0 or 1, other values QEC_ERR_ARG): the order of min-sum's updates.  0 = flooding,
 *     as ever (the same kernels).  1 = layered (check-sequential) min-sum, DESIGN.md section 2, "The layered min-sum
 *     form": the state is one fp32 check->variable LLR R per real edge, +0.0f at the start (an unused slot of a general
 *     code reads +0.0f in q_final).  An iteration takes the sector's checks in the order of qec_code_layers, sorted by
 *     (colour, index); check c forms, for each of its slots in ascending order, the left fold lambda_v + R of v's OTHER
 *     checks as they stand, in ascending check order, and then its own R by the check update of QEC_OPT_BP_METHOD = 1
 *     (a check of degree 1 sends alpha * 2^20).  The posterior of v is the same fold over ALL its checks; its decision
 *     is posterior < 0.0f; a variable in no check decides 0 and enters no test.  Stop rules over the posteriors: FIXED N
 *     iterations; SYNDROME after the first iteration whose decisions satisfy the syndrome; REF after an iteration with
 *     index % 10 == 0 that leaves no posterior inside (fabsf < 4.5951198f).  There is no special last iteration.
 *     CONVERGENCE_FAIL: a posterior of the final state inside; SYNDROME_FAIL from the final decisions; q_final: every
 *     real slot of v holds v's final posterior; N = 0 gives lambda_v.  The value is data, like QEC_OPT_MINSUM_SCALE: it
 *     is read at every decode call and takes effect while QEC_OPT_BP_METHOD = 1 and no relay tables are set; under the
 *     product rule it does nothing, and a relay runs its flooding legs as before.  QEC_OPT_BP_SCHEDULE is the product
 *     rule's serial schedule and stays what it was: it and QEC_OPT_BP_METHOD = 1 still refuse each other.  Sparse-graph
 *     engine (the LAYERED kernels of bp_sparse.hip; plan, workspace, grid and describe string unchanged; the layer
 *     tables are uploaded when the plan is created, so setting the option allocates nothing) and CPU engine; a
 *     wave-circulant handle refuses 1 with QEC_ERR_UNSUPPORTED and the text says to create the decoder with
 *     QEC_ENGINE_SPARSE.  With QEC_OPT_MINSUM_WAVE = 1 a layered decode runs the layered wave kernels of
 *     bp_wave_minsum.hip ("The layered min-sum form in the wave layout": the messages in the
 *     variable view, a layer = a block row = one lane-local check pass; no LDS, no barrier, no scratch), bit for bit
 *     the LAYERED kernels' outputs.  QEC_OPT_LAST_PATH carries QEC_PATH_MINSUM | QEC_PATH_SERIAL when the layered rule
 *     ran, and QEC_PATH_WAVE beside them when the wave kernels ran it.  Every decode entry point
 *     honours it, the _dev ones read it at the call and allocate nothing (a captured graph keeps the kernels it
 *     captured); the OSD stage's soft decode runs the same schedule (its column key reads q_final, here the
 *     posterior).  The near-hard jump never fires.  A schedule for the QC codes: on the hypergraph product hgp_ham it
 *     leaves more syndromes unsatisfied than flooding min-sum does (README).  A group applies the value to every part.
 *   QEC_OPT_LIGHT_MEMO (default 1; fixed and reference stop, no q_final requested; the wave-circulant kernels of
 *     one-syndrome-per-wave codes with generated shifts, i.e. P61): a sector whose syndrome is that of one qubit
 *     error, or of two whose checks are disjoint, takes its outcome from a table instead of decoding.  The update
 *     rules of a quasi-cyclic code do not depend on the lane, so the outcome of such a sector depends only on its
 *     class (the column, or both columns and the lane difference); the decoder's own kernels decode one
 *     representative per class once per key (p', N, stop rule), on the stream of the first call that uses the key,
 *     without synchronising; an entry is used only where that decode returned exactly the generating qubits with
 *     both flags clear.  The table and the fill's workspace (about 22 MB for P61) are allocated by
 *     qec_decoder_create.  A call captured into a graph while its key is cold runs without the table.  Every
 *     output bit identical either way; 0 decodes those sectors by BP (for measurement).  Each part of a group
 *     holds its own table.
 *   QEC_OPT_NEAR_PROBE (default 1; needs QEC_OPT_NEAR_HARD_JUMP; the fixed- and reference-stop kernels of P61): the
 *     soft iteration that could end a sector first tests the two folds t0, t1 of every outgoing message
 *     q = t1 / (t0 + t1) instead of dividing (qec_near_probe): one at least 2 / eps0 times the other on every edge,
 *     each variable's on one side, and those sides satisfy the syndrome.  That implies the jump's exact test with
 *     the same sides, so the sector leaves without forming or returning a message; where
 *     the probe fails the ordinary pass runs and its exact test decides, in the same iteration as before.  Every
 *     output bit identical either way; 0 always takes the ordinary pass (for measurement).  The CPU engine keeps
 *     the exact test. */
enum { QEC_OPT_HARD_PATHS = 1, QEC_OPT_CYCLE_JUMP = 2, QEC_OPT_SCHEDULE = 3, QEC_OPT_SECTOR_SPLIT = 4,
       QEC_OPT_PHASE_STATS = 5, QEC_OPT_TRIAGE = 6, QEC_OPT_LAST_PATH = 7, QEC_OPT_MC_DECODE_TIME = 8,
       QEC_OPT_OSD = 9, QEC_OPT_OSD_ITERATIONS = 10, QEC_OPT_OSD_SECTORS = 11, QEC_OPT_OSD_SWEEP = 12,
       QEC_OPT_OSD_ORDER = 13, QEC_OPT_OSD_CS_SECTORS = 14, QEC_OPT_NEAR_HARD_JUMP = 15, QEC_OPT_OSD_SCORE = 16,
       QEC_OPT_CORRELATED = 17, QEC_OPT_BP_SCHEDULE = 18, QEC_OPT_BP_METHOD = 19, QEC_OPT_MINSUM_SCALE = 20,
       QEC_OPT_MINSUM_WAVE = 21, QEC_OPT_RELAY_WAVE = 22, QEC_OPT_MINSUM_SCHEDULE = 23, QEC_OPT_LIGHT_MEMO = 24,
       QEC_OPT_NEAR_PROBE = 25 };
enum {
    QEC_PATH_ORDERED = 1,          /* dispatch order pass (schedule.hip) */
    QEC_PATH_SECTOR_ORDER = 2,     /* ... in the per-sector form (each sector's waves by its own weight) */
    QEC_PATH_SPLIT_WAVES = 4,      /* X and Z sectors in separate waves of one launch */
    QEC_PATH_SECTOR_LAUNCHES = 8,  /* an X launch, then a Z launch */
    QEC_PATH_TRIAGE = 16,          /* iteration-0 triage + list-mode decode */
    QEC_PATH_BIT_ROWS = 32,        /* bit-row syndromes in */
    QEC_PATH_SPARSE = 64,          /* sparse-graph engine */
    QEC_PATH_RECORDS = 128,        /* packed decision records out */
    QEC_PATH_OSD = 256,            /* the call ran the OSD stage (QEC_OPT_OSD) */
    QEC_PATH_CORRELATED = 512,     /* one sector decoded under priors conditioned on the other's estimate */
    QEC_PATH_SERIAL = 1024,        /* BP under the serial schedule (QEC_OPT_BP_SCHEDULE = 1), or layered min-sum
                                      (QEC_OPT_MINSUM_SCHEDULE = 1, then beside QEC_PATH_MINSUM) */
    QEC_PATH_MINSUM = 2048,        /* scaled min-sum BP (QEC_OPT_BP_METHOD = 1) */
    QEC_PATH_RELAY = 4096,         /* ... as a relay of memory min-sum legs (qec_decoder_set_relay) */
    QEC_PATH_SOFT = 16384,         /* ... under syndrome priors (qec_decoder_set_syndrome_priors) */
    QEC_PATH_WAVE = 8192           /* ... by the register-resident wave kernels (QEC_OPT_MINSUM_WAVE = 1, or
                                      QEC_OPT_RELAY_WAVE = 1 on a relay decode) */
};
/* The near-hard jump's threshold for p' = pPrime (the float (2/3) errorProbability the decoder forms), R
 * checks per variable and L variables per check: *eps0 = the largest power of two in [2^-20, 2^-8] with
 * 2 ((1 - p') / p') (delta / (1 - delta))^(R - 1) <= eps0, delta = (L - 1) eps0 + 2^-20 (evaluated in double),
 * or 0 if there is none or p' is outside (0, 1/2] (the jump then never fires); *T = the bit pattern one below
 * the float eps0 (1 - eps0): bits(fma(-q, q, q)) <= T as unsigned integers implies q <= eps0 or q >= 1 - eps0. */
int qec_near_hard_threshold(float pPrime, int R, int L, float* eps0, uint32_t* T);
/* The near-hard probe's test of one outgoing message q = t1 / (t0 + t1) from its two folds, for eps0 a power of two
 * in [2^-20, 2^-8] (else 0): returns 1 iff both bit patterns lie below 0x7F000000 (non-negative, no -0, below
 * 2^127, no NaN) and differ by at least (k + 1) << 23, eps0 = 2^-k -- which implies that the larger fold is at
 * least 2 / eps0 times the smaller, exactly that on normal floats -- and then *side (nullable) = 1 iff t1 > t0.  A
 * pair that passes has q' = RN(t1 / RN(t0 + t1)) with bits(fma(-q', q', q')) <= T of qec_near_hard_threshold and
 * (q' >= 0.5f) == *side. */
int qec_near_probe(float t0, float t1, float eps0, int* side);
int qec_decoder_set_option(qec_decoder* dec, int option, int value);
int qec_decoder_get_option(const qec_decoder* dec, int option, int* value);
/* Per-qubit error priors ("prior form"): biased noise, qubits of different quality,
 * erasures (prior 1/2), measurement-error columns with their own rate.  priorX, priorZ: HOST arrays of n
 * floats; priorX[v] is the prior that bit v of the X-sector estimate (eX) is 1, priorZ[v] the same for eZ.
 * While priors are set, a sector's BP starts every real slot of variable v at pi_v (unused slots of a general
 * code stay +0.0f) and starts v's two running products from 1.0f - pi_v and pi_v, where the scalar form uses
 * 1 - p' and p' = (2/3) errorProbability; operation order, check update, stop rules, flags, iteration counts,
 * decisions and the q_final layout are untouched.  With every pi_v equal to the float 2.0f / 3.0f * p every
 * output bit equals the scalar call at p.
 *   - The errorProbability argument of EVERY decode entry point (qec_decode_batch, _dev, _packed, _packed_dev,
 *     qec_get_statistics, qec_monte_carlo, the OSD stage's soft decode) is then NOT USED by BP; it must still
 *     be a valid float.
 *   - Both NULL clears the priors: the handle behaves exactly as one that never had any (the same kernels).
 *     Exactly one NULL: QEC_ERR_ARG.  Every entry must satisfy 0 <= pi <= 1 (0, 0.5 and 1 are legal; NaN is
 *     not): QEC_ERR_ARG otherwise, and the error text names the sector and index ("priorZ[17] = ...").
 *   - Synchronous: waits for the handle's last launch, then copies the priors to the device.  The device
 *     buffer is allocated by the first set and rewritten in place afterwards, so the _dev decode entry points
 *     keep their contract (no allocation, no synchronisation) and stay graph-capturable with priors set; a
 *     captured graph replayed after a later set decodes with the new values.
 *   - Engines: the sparse-graph engine (regular and general codes) and the CPU engine take priors.  A
 *     wave-circulant handle refuses with QEC_ERR_UNSUPPORTED -- its hard-message shortcuts and their thresholds
 *     are proven for one p' -- and the text says to create the decoder with QEC_ENGINE_SPARSE.
 *     qec_decode_bits_packed_dev is wave-circulant only and so never sees priors.  On a group the priors apply
 *     to every part.
 *   - The near-hard jump (QEC_OPT_NEAR_HARD_JUMP) of the CPU engine never fires while priors are set (its lemma
 *     is stated for one p'); outputs do not depend on the jump either way.
 *   - OSD (QEC_OPT_OSD, QEC_OPT_OSD_ORDER): the soft decode that orders the columns runs with the priors.  The
 *     combination sweep scores its candidates by Hamming weight by default (QEC_OPT_OSD_SCORE = 0) and, with
 *     QEC_OPT_OSD_SCORE = 1, by likelihood under the priors: the sum of the integer weights w(pi_v) of the
 *     flipped qubits, least sum first.  Every set rebuilds the two weight tables (and rewrites their device
 *     copy in place, allocated by the first set as the priors' own buffer is, so qec_osd_dev stays free of
 *     allocation and synchronisation and a captured graph replayed after a later set scores with the new
 *     tables).  The stage's result depends on (code, syndrome, priors, QEC_OPT_OSD_ITERATIONS, lambda,
 *     QEC_OPT_OSD_SCORE) only.
 *   - qec_sample_syndrome_dev and qec_monte_carlo then draw their errors from the independent sampler of
 *     qec_sample_independent_dev (their scalar p is not used), and qec_monte_carlo takes the unfused pipeline
 *     with byte syndromes (sample + syndromes + packed errors, packed decode, OSD stage if on, statistics),
 *     the sequence QEC_OPT_OSD already forces; the counters describe that run. */
int qec_decoder_set_priors(qec_decoder* dec, const float* priorX, const float* priorZ);
/* 1 and the arrays filled (n floats each; a NULL array is skipped) if priors are set, 0 if not. */
int qec_decoder_get_priors(const qec_decoder* dec, float* priorX, float* priorZ);
/* The combination sweep's weight tables under QEC_OPT_OSD_SCORE = 1 (built by qec_decoder_set_priors whatever
 * the option's value): 1 and the arrays filled (n entries each, 0 .. 4095; a NULL array is skipped) if
 * priors are set, 0 if not. */
int qec_decoder_get_osd_weights(const qec_decoder* dec, int32_t* wX, int32_t* wZ);
/* The channel LLR of the min-sum form (QEC_OPT_BP_METHOD = 1) for a prior pi: *llr = (float) log((1 - pi) / pi),
 * the float taken exactly to double and the result rounded once, clamped to [-2^30, +2^30]: pi = 0 gives
 * +1073741824.0f, pi = 1 gives -1073741824.0f and pi = 1/2 gives +0.0f.  Both engines decode with exactly these
 * values. */
int qec_minsum_llr(float prior, float* llr);
/* The channel LLR tables that every qec_decoder_set_priors builds (whatever QEC_OPT_BP_METHOD says): the arrays
 * filled (n floats each; a NULL array is skipped).  QEC_ERR_ARG if no priors are set. */
int qec_decoder_get_minsum_llr(const qec_decoder* dec, float* llrX, float* llrZ);
/* Relay-BP ("The relay form"): min-sum with one fp32 memory M_v per variable, run as a chain of
 * `legs` legs; a message-passing-only route to the syndromes that plain BP leaves unsatisfied.  gammaX, gammaZ: HOST
 * tables [legs][n] of memory strengths, each finite with |gamma| <= 1 (negative values are legal); solutions = S, the
 * solutions to collect.  1 <= legs <= 1024 with legs * n <= 2^22, 1 <= S <= 64; an illegal value gives QEC_ERR_ARG and
 * leaves the handle as it was.  (NULL, NULL, 0, 0) clears: the handle behaves as one that never had tables.
 *   - The tables are data, like QEC_OPT_MINSUM_SCALE: they take effect in every decode while QEC_OPT_BP_METHOD = 1 and
 *     have no effect under the product rule.  Everything not said here is the min-sum form (channel LLRs, check
 *     update, K, alpha, the inside band, flags, layout).  X and Z relay independently.
 *   - Leg 0 starts with M_v = lambda_v, leg l >= 1 with the posteriors of leg l - 1's last variable pass; every leg
 *     starts with every real slot at its variable's lambda_v.  Variable update, every operation fp32 and uncontracted:
 *     b = ((1.0f - gamma) * lambda_v + gamma * M_v) + 0.0f takes lambda_v's place in the folds, and M_v = the
 *     posterior.  The call's stop rule and maxIter = N end a leg, counted within the leg.
 *   - A leg whose final decisions satisfy the syndrome is a solution of weight W = sum of w_v over its set bits (an
 *     unsigned 32-bit sum; w_v = 1, or with priors the entry of qec_decoder_get_osd_weights).  The sector ends at its
 *     S-th solution or after its last leg and returns the solution of least W (ties: the earlier leg), or without a
 *     solution the last leg's decisions with SYNDROME_FAIL set.  CONVERGENCE_FAIL and q_final describe the last executed
 *     leg's final state, iters counts the iterations of all legs; N = 0 runs one leg and equals min-sum's N = 0.
 *     With legs = 1 and every gamma = 0 every output bit equals the plain min-sum call.
 *   - Engines: the sparse-graph engine (the RELAY kernels of bp_sparse.hip; plan, workspace, grid and describe string
 *     unchanged) and the CPU engine.  A wave-circulant handle refuses with QEC_ERR_UNSUPPORTED and the text says to
 *     create the decoder with QEC_ENGINE_SPARSE.  A group passes the tables to every part.
 *   - Synchronous.  The first set allocates the device copy (at its largest legal size, so no later set moves it) and
 *     the kernels' per-workgroup state; qec_decoder_set_option and the _dev entry points allocate nothing, and a
 *     captured graph replayed after a later set reads the new table values (legs and S as captured).
 *   - QEC_PATH_RELAY is set in QEC_OPT_LAST_PATH whenever the relay ran.  The OSD stage runs behind it on the sectors
 *     it leaves failed; the stage's own soft decode ignores the tables (plain min-sum). */
int qec_decoder_set_relay(qec_decoder* dec, const float* gammaX, const float* gammaZ, int legs, int solutions);
/* *legs and *solutions (0 and 0 without tables; a NULL pointer is skipped) and, where given, the tables ([legs][n]). */
int qec_decoder_get_relay(const qec_decoder* dec, float* gammaX, float* gammaZ, int* legs, int* solutions);
/* Noisy syndromes ("The soft-syndrome form"): qX [numEqsX], qZ [numEqsZ] are HOST arrays, q_c = the
 * probability that the measured bit of check c is flipped.  Every entry in [0, 1] (NaN is not): QEC_ERR_ARG otherwise,
 * and for exactly one NULL pointer; the handle is then unchanged.  (NULL, NULL) clears: the handle behaves as one that
 * never had them.
 *   - Decoding (H, s) under syndrome priors is decoding the extended code [H | I] whose variable n + c sits in check c
 *     only, with channel LLR mu_c = qec_minsum_llr(q_c); the outputs are those of the first n variables and the real
 *     slots of H.  Natively: check c has one virtual input mu_c in every check pass, the virtual slot's output rho_c gives
 *     the measurement decision f_c = (mu_c + rho_c < 0.0f) (before the first check pass f_c = mu_c < 0.0f), and the
 *     syndrome test (the syndrome stop and SYNDROME_FAIL) compares (parity of the row's decisions) ^ f_c with the entry.
 *     The inside tests (the reference stop, CONVERGENCE_FAIL) look at the data slots / data posteriors only.  With every
 *     q_c = 0 every output bit equals the call without syndrome priors.
 *   - They are a form of plain min-sum, flooding or layered (QEC_OPT_MINSUM_SCHEDULE), on the sparse-graph engine (the
 *     SOFT kernels of bp_sparse.hip, or with QEC_OPT_MINSUM_WAVE = 1 those of bp_wave_minsum.hip) and the CPU engine.  Every decode entry point of such a handle decodes under them
 *     (qec_decode_batch*, the _dev and packed forms, qec_get_statistics, qec_monte_carlo) with unchanged output layouts,
 *     and QEC_PATH_SOFT is then set in QEC_OPT_LAST_PATH; qec_decoder_describe appends " [soft syndrome]".
 *   - Refusals, QEC_ERR_UNSUPPORTED with the handle unchanged, whichever call comes second: they need
 *     QEC_OPT_BP_METHOD = 1 and that option refuses 0 while they are set; they and relay tables (qec_decoder_set_relay)
 *     refuse each other; they and QEC_OPT_OSD = 1 refuse each other (OSD solves H e = s exactly; qec_osd and qec_osd_dev
 *     as separate calls are untouched); a wave-circulant handle refuses them.
 *   - Synchronous.  The first set allocates the device copy, later sets rewrite it in place; the _dev entry points
 *     allocate nothing, and a captured graph replayed after a later set decodes with the new values.  A group passes
 *     the tables to every part. */
int qec_decoder_set_syndrome_priors(qec_decoder* dec, const float* qX, const float* qZ);
/* 1 and the arrays filled (a NULL array is skipped) if syndrome priors are set, 0 if not. */
int qec_decoder_get_syndrome_priors(const qec_decoder* dec, float* qX, float* qZ);
/* The scalar tables of QEC_OPT_CORRELATED for depolarising noise of strength p: *c1 = P(other bit | this bit
 * set) = 0.5f and *c0 = P(other bit | this bit clear) = (p / 3.0f) / (1.0f - 2.0f / 3.0f * p), every operation
 * in fp32.  Both engines decode with exactly these values. */
int qec_correlated_priors(float p, float* c0, float* c1);
/* Per-qubit Pauli channel: qubit v suffers X, Y or Z with probabilities pX[v], pY[v], pZ[v] (HOST arrays of n
 * floats); Y sets both bits.  Every entry in [0, 1] (NaN is not), (pX + pY) + pZ <= 1 evaluated in double:
 * QEC_ERR_ARG otherwise, the text names array and index ("pY[17] = ...", "pX[17] + pY[17] + pZ[17] = ...").  Exactly one
 * or two NULL pointers: QEC_ERR_ARG; all three NULL clears the channel and the priors.
 *   - Marginals: priorX = pX + pY, priorZ = pZ + pY (double from the floats, rounded once to float), installed
 *     exactly as qec_decoder_set_priors(priorX, priorZ) installs them (device buffer, OSD weight tables, its
 *     refusals, every part of a group); qec_decoder_get_priors returns them.
 *   - Conditionals (double, one rounding, min(1, .); a zero denominator gives 0.5f): cZ1 = pY / (pX + pY),
 *     cZ0 = pZ / (1 - (pX + pY)), cX1 = pY / (pZ + pY), cX0 = pX / (1 - (pZ + pY)): the priors of the second
 *     sector's bit given the first sector's estimate under QEC_OPT_CORRELATED.
 *   - Any later qec_decoder_set_priors, (NULL, NULL) included, drops the channel.
 *   - The device copies follow the priors' contract: allocated by the first set, rewritten in place afterwards,
 *     synchronous; the _dev entry points allocate nothing and never synchronise, and a captured graph replayed
 *     after a later set decodes (and samples) with the new tables.
 *   - On a handle with a channel qec_sample_syndrome_dev and qec_monte_carlo draw qec_sample_pauli_dev's errors,
 *     whatever QEC_OPT_CORRELATED says (the channel is the noise, the option how it is decoded), through the
 *     unfused byte-syndrome pipeline that priors force.
 *   - A wave-circulant handle refuses with QEC_ERR_UNSUPPORTED (create the decoder with QEC_ENGINE_SPARSE). */
int qec_decoder_set_pauli_channel(qec_decoder* dec, const float* pX, const float* pY, const float* pZ);
/* 1 and the arrays filled (n floats each; a NULL array is skipped) if a channel is set, 0 if not. */
int qec_decoder_get_pauli_channel(const qec_decoder* dec, float* pX, float* pY, float* pZ);
int qec_decoder_get_conditional_priors(const qec_decoder* dec, float* cZ0, float* cZ1, float* cX0, float* cX1);
/* which kernel variant serves this code: writes a short name (e.g. "wave-circulant P=61 G=1") */
int qec_decoder_describe(const qec_decoder* dec, char* buf, size_t len);

/* Batched Decoder::Decode (QEC_LDPC/Decoder.h:40-41, semantics of
 * DecoderCPU::Decode, DecoderCPU.h:317-390) on HOST buffers; synchronous.
 *   sX: B x numEqsX, sZ: B x numEqsZ   syndromes (0/1 bytes)
 *   eX, eZ: B x n                      decoded error estimates (0/1 bytes)
 *   flags: B                           ErrorCode bits per syndrome pair
 *   iters: B x 2 (optional)            BP iterations executed (X, Z)
 *   q_final: B x (numEqsX+numEqsZ) x L (optional) final variable->check messages,
 *            [check][slot] with slots in ascending variable order (X block first).
 *            A general code (qec_code_from_matrices): the stride is D of qec_code_degrees
 *            instead of L, B x (numEqsX+numEqsZ) x D; a check of lower weight leaves its
 *            last slots unused, written as +0.0f
 * errorProbability / maxIterations as in Decode; stop = QEC_STOP_*.
 * On a handle with priors (qec_decoder_set_priors) BP uses them and errorProbability is NOT USED, here and
 * in qec_decode_batch_dev, qec_decode_batch_packed, qec_decode_batch_packed_dev, qec_get_statistics and
 * qec_monte_carlo (it must still be a valid float). */
int qec_decode_batch(qec_decoder* dec, const uint8_t* sX, const uint8_t* sZ, size_t B,
                     float errorProbability, int maxIterations, int stop,
                     uint8_t* eX, uint8_t* eZ, uint8_t* flags, int32_t* iters, float* q_final);
/* Same on DEVICE buffers (same layouts), enqueued on `stream` (hipStream_t or NULL),
 * asynchronous: no host synchronisation, no allocation (graph-capturable). */
int qec_decode_batch_dev(qec_decoder* dec, const uint8_t* sX, const uint8_t* sZ, size_t B,
                         float errorProbability, int maxIterations, int stop,
                         uint8_t* eX, uint8_t* eZ, uint8_t* flags, int32_t* iters, float* q_final,
                         void* stream);
/* qec_decode_batch and qec_decode_batch_dev with the measurement decisions of a handle with syndrome priors
 * (qec_decoder_set_syndrome_priors) as two further nullable outputs: fX [B x numEqsX] and fZ [B x numEqsZ] bytes,
 * f = 1 where the decoder takes the measured syndrome bit as flipped.  Any min-sum handle (QEC_OPT_BP_METHOD = 1;
 * QEC_ERR_UNSUPPORTED otherwise); without syndrome priors f is all zero.  Every other output equals the plain call's.
 * The _dev form allocates nothing and is graph-capturable. */
int qec_decode_batch_soft(qec_decoder* dec, const uint8_t* sX, const uint8_t* sZ, size_t B,
                          float errorProbability, int maxIterations, int stop,
                          uint8_t* eX, uint8_t* eZ, uint8_t* fX, uint8_t* fZ, uint8_t* flags, int32_t* iters,
                          float* q_final);
int qec_decode_batch_soft_dev(qec_decoder* dec, const uint8_t* sX, const uint8_t* sZ, size_t B,
                              float errorProbability, int maxIterations, int stop,
                              uint8_t* eX, uint8_t* eZ, uint8_t* fX, uint8_t* fZ, uint8_t* flags, int32_t* iters,
                              float* q_final, void* stream);
/* The measurement-error channel of a handle with syndrome priors, in place on DEVICE byte syndromes sX [B x numEqsX],
 * sZ [B x numEqsZ]; fX / fZ (nullable, same shapes) receive the flips.  Sample b (index start + b) makes Philox4x32-10
 * calls k = 0, 1, ... with counter (b lo, b hi, k, 0xA54FF53A) and key (seed lo, seed hi); word 4k + j is output j of
 * call k; X check c reads word c, Z check c word numEqsX + c; the bit is flipped iff word < floor(q 2^32), evaluated in
 * double from the float as a 64-bit value (q = 1 always flips, q = 0 never).  Any shard of the index space can be drawn
 * alone.  QEC_ERR_ARG without syndrome priors.  On such a handle qec_sample_syndrome_dev and qec_monte_carlo apply
 * these flips after the syndrome, with the same seed and sample index (errp stays the data error). */
int qec_flip_syndrome_dev(qec_decoder* dec, uint64_t seed, uint64_t start, size_t B, uint8_t* sX, uint8_t* sZ,
                          uint8_t* fX, uint8_t* fZ, void* stream);
/* Bit-packed output (SURVEY.md 8(d)'s I/O model): the decode kernel writes one decision record
 * per syndrome instead of eX / eZ / flags: records is B x QEC_RECORD_BYTES(n) bytes, per syndrome
 * eX packed (ceil(n/8) bytes, bit j of byte k = qubit 8k + j, padding bits 0), then eZ packed,
 * then the ErrorCode flags byte.  Same decisions bit for bit as the byte form. */
#define QEC_RECORD_BYTES(n) (2 * (((n) + 7) / 8) + 1)
int qec_decode_batch_packed_dev(qec_decoder* dec, const uint8_t* sX, const uint8_t* sZ, size_t B,
                                float errorProbability, int maxIterations, int stop,
                                uint8_t* records, int32_t* iters, float* q_final, void* stream);
/* The same with bit-row syndromes (the Monte-Carlo pipeline's layout, 72 instead of 549 bytes per
 * P61 syndrome): sXbits [B][ceil(numEqsX / 32)] and sZbits [B][ceil(numEqsZ / 32)] 32-bit words,
 * bit c of a row = check c (bit c % 32 of word c / 32).  Wave-circulant engine only
 * (QEC_ERR_UNSUPPORTED otherwise).  Under the syndrome stop this is the entry point that takes
 * the triage (QEC_OPT_TRIAGE) when no final messages are requested. */
int qec_decode_bits_packed_dev(qec_decoder* dec, const uint32_t* sXbits, const uint32_t* sZbits, size_t B,
                               float errorProbability, int maxIterations, int stop,
                               uint8_t* records, int32_t* iters, float* q_final, void* stream);
/* Host-buffer form of the packed decode (synchronous). */
int qec_decode_batch_packed(qec_decoder* dec, const uint8_t* sX, const uint8_t* sZ, size_t B,
                            float errorProbability, int maxIterations, int stop,
                            uint8_t* records, int32_t* iters);

/* ---- Monte-Carlo caller side (DecoderCPU::GetStatistics, DecoderCPU.h:392-530) */
/* The reference's fixed-weight sampler (DecoderCPU.h:448-459, RandomErrorGenerator.h:31-44):
 * one mt19937(seed) stream, VS2015 uniform_int_distribution, W x (index, type) draws per
 * sample.  x, z: count x n (0/1). */
int qec_sample_fixed_weight(uint32_t seed, int W, size_t count, int n, uint8_t* x, uint8_t* z);
/* Decoder::GetStatistics(errorWeight, numErrors, errorProbability, maxIterations, seed)
 * (Decoder.h:44-47): samples numErrors errors exactly as the reference does, decodes them on
 * the GPU (reference stop rule) and fills the CodeStatistics counters.  The reference tests
 * (numErrors / nThreads) * nThreads samples; pass nThreads = 1 to test all numErrors. */
int qec_get_statistics(qec_decoder* dec, int errorWeight, int numErrors, float errorProbability,
                       int maxIterations, uint32_t seed, int nThreads, qec_stats* out);

/* ---- Monte-Carlo on the device (the GetStatistics loop, batched) ---- */
/* counters in device order for qec_statistics_dev */
enum { QEC_MC_WITHX, QEC_MC_WITHZ, QEC_MC_SYNX, QEC_MC_SYNZ, QEC_MC_LOGICAL, QEC_MC_CORRECTED, QEC_MC_CONVX,
       QEC_MC_CONVZ, QEC_MC_NCOUNTERS,
       /* qec_statistics_packed_dev with iters: BP iterations executed, summed per sector */
       QEC_MC_ITERX = QEC_MC_NCOUNTERS, QEC_MC_ITERZ, QEC_MC_NCOUNTERS_ALL };

typedef struct {
    uint64_t tested, withX, withZ, synX, synZ, logical, corrected, convX, convZ;
    uint64_t iterationsX, iterationsZ; /* BP iterations executed, summed over samples */
    double decodeSeconds;             /* decode-kernel time (HIP events), summed over batches */
    double totalSeconds;              /* wall time of the call */
} qec_mc_result;

/* i.i.d. depolarising errors for samples [start, start+B) of stream `seed` (device buffers
 * x, z: B x n).  Each qubit is hit with probability thr / 2^32, thr = floor(p 2^32) (saturated),
 * independently, drawn as a walk over the gaps between hits: sample b reads 32-bit words from
 * Philox4x32-10 calls k = 0, 1, ... (counter (b lo, b hi, k, 0x6A9C0DE5), key (seed lo, seed hi),
 * word 4k + j = output word j of call k); u = next word skips G = #{g in 1..n : u < T[g]} qubits,
 * T[g] = floor(q^g 2^32), q = 1 - thr / 2^32 (q^g by right-to-left binary exponentiation in IEEE
 * double); a qubit still inside the sample is then hit, of type floor(3 w / 2^32) of the next word
 * w: 0 = X, 1 = Y, 2 = Z (Y sets both bits).  Any shard of the index space can be drawn alone. */
int qec_sample_depolarizing_dev(qec_decoder* dec, uint64_t seed, uint64_t start, size_t B, float p, uint8_t* x,
                                uint8_t* z, void* stream);
/* Independent X / Z errors over the handle's priors (qec_decoder_set_priors; QEC_ERR_ARG without them) for
 * samples [start, start+B) of stream `seed` (device buffers x, z: B x n bytes).  Sample b makes
 * Philox4x32-10 calls k = 0, 1, ... with counter (b lo, b hi, k, 0x51ED270B) and key (seed lo, seed hi); word
 * 4k + j is output word j of call k; x[v] = (word 2v < thrX[v]) and z[v] = (word 2v + 1 < thrZ[v]) with
 * thr = floor(pi 2^32), evaluated in double from the float, as a 64-bit value: pi = 1 gives 2^32 and always
 * hits, pi = 0 never hits.  Any shard of the index space can be drawn alone.  Enqueued on `stream`; no
 * synchronisation, no allocation.  Single-device GPU handle. */
int qec_sample_independent_dev(qec_decoder* dec, uint64_t seed, uint64_t start, size_t B, uint8_t* x, uint8_t* z,
                               void* stream);
/* Errors of the handle's Pauli channel (qec_decoder_set_pauli_channel; QEC_ERR_ARG without one) for samples
 * [start, start+B) of stream `seed` (device buffers x, z: B x n bytes).  Sample b makes Philox4x32-10 calls
 * k = 0, 1, ... with counter (b lo, b hi, k, 0x3C6EF372) and key (seed lo, seed hi); output word j of call k is
 * the word u of qubit 4k + j.  With the 64-bit thresholds tX = floor(pX 2^32), tXY = floor((pX + pY) 2^32) and
 * tXYZ = floor(min(1, (pX + pY) + pZ) 2^32), evaluated in double from the floats: x = u < tXY and
 * z = tX <= u < tXYZ.  Any shard of the index space can be drawn alone.  Enqueued on `stream`; no
 * synchronisation, no allocation.  Single-device GPU handle. */
int qec_sample_pauli_dev(qec_decoder* dec, uint64_t seed, uint64_t start, size_t B, uint8_t* x, uint8_t* z,
                         void* stream);
/* Fused front end: the depolarising errors of qec_sample_depolarizing_dev (same stream, same
 * bits) go straight to their syndromes (GetSyndromeX/Z, Quantum_LDPC_Code.h:94-124) without
 * leaving the chip: sX B x numEqsX, sZ B x numEqsZ, and optionally errp B x 2 ceil(n/8), the
 * errors bit-packed in the decision-record layout (x bits then z bits) for
 * qec_statistics_packed_dev.  One wave per sample.  On a handle with priors the errors are those of
 * qec_sample_independent_dev instead (same stream, same bits) and p is not used; with a Pauli channel those of
 * qec_sample_pauli_dev. */
int qec_sample_syndrome_dev(qec_decoder* dec, uint64_t seed, uint64_t start, size_t B, float p, uint8_t* sX,
                            uint8_t* sZ, uint8_t* errp, void* stream);
/* GetSyndromeX/Z (Quantum_LDPC_Code.h:94-124) of device error vectors: x, z B x n -> sX B x numEqsX, sZ B x numEqsZ */
int qec_syndrome_dev(qec_decoder* dec, const uint8_t* x, const uint8_t* z, size_t B, uint8_t* sX, uint8_t* sZ,
                     void* stream);
/* The CodeStatistics counters of a decoded device batch (DecoderCPU.h:464-521: errors present,
 * syndrome fails, I-P logical check when neither syndrome failed, convergence fails), ADDED to
 * the device array counters[QEC_MC_NCOUNTERS] (uint64). */
int qec_statistics_dev(qec_decoder* dec, const uint8_t* x, const uint8_t* z, const uint8_t* eX, const uint8_t* eZ,
                       const uint8_t* flags, size_t B, uint64_t* counters, void* stream);
/* The same counters from packed errors (qec_sample_syndrome_dev's errp) and packed decision
 * records (qec_decode_batch_packed_dev), ADDED to counters[QEC_MC_NCOUNTERS], or, with iters
 * (B x 2, nullable) given, to counters[QEC_MC_NCOUNTERS_ALL] including the iteration sums. */
int qec_statistics_packed_dev(qec_decoder* dec, const uint8_t* errp, const uint8_t* records, const int32_t* iters,
                              size_t B, uint64_t* counters, void* stream);
/* Per-sample form of qec_statistics_packed_dev's logical / corrected split: errp B x 2 ceil(n/8),
 * records B x QEC_RECORD_BYTES(n) (any base alignment), outcome B bytes: QEC_OUTCOME_SYNDROME_FAIL
 * if the record's flags carry a syndrome failure, else QEC_OUTCOME_LOGICAL if the residual
 * errp ^ record fails the code's logical check, else QEC_OUTCOME_CORRECTED (convergence bits do not
 * matter).  Enqueued on `stream`; no synchronisation, no allocation, nothing written but outcome[0, B).
 * GPU engines, single-device handle, code with a logical check, 2n <= 4096. */
enum { QEC_OUTCOME_CORRECTED = 0, QEC_OUTCOME_LOGICAL = 1, QEC_OUTCOME_SYNDROME_FAIL = 2 };
int qec_logical_packed_dev(qec_decoder* dec, const uint8_t* errp, const uint8_t* records, size_t B,
                           uint8_t* outcome, void* stream);
/* OSD (QEC_OPT_OSD above, steps "order" to "flag"; the handle's QEC_OPT_OSD_ORDER chooses OSD-0 or the
 * combination sweep, read at the call as QEC_OPT_OSD_SWEEP is) in place on a decoded DEVICE batch: sX, sZ, eX,
 * eZ, flags in the layouts of qec_decode_batch_dev, q the soft input in the q_final layout (B x
 * (numEqsX+numEqsZ) x L; any decode's q_final: the caller chooses the iterations).  Sectors without
 * their SYNDROME_FAIL bit are skipped.  Enqueued on `stream`: no synchronisation, no allocation
 * (graph-capturable); nothing is written but the repaired sectors' rows of eX / eZ and their bits of
 * flags[0, B).  Single-device GPU handle.  Updates neither QEC_OPT_OSD_SECTORS nor
 * QEC_OPT_OSD_CS_SECTORS. */
int qec_osd_dev(qec_decoder* dec, const uint8_t* sX, const uint8_t* sZ, size_t B, const float* q,
                uint8_t* eX, uint8_t* eZ, uint8_t* flags, void* stream);
/* The same on HOST buffers, synchronous, on any engine (the CPU engine runs the host implementation,
 * osd_host.cpp; a GPU handle the kernel). */
int qec_osd(qec_decoder* dec, const uint8_t* sX, const uint8_t* sZ, size_t B, const float* q,
            uint8_t* eX, uint8_t* eZ, uint8_t* flags);
/* Decision records for gathering a sharded batch to one rank (the decoded
 * vectors travel bit-packed): out is B x (2 ceil(n/8) + 1) bytes, per syndrome eX packed
 * (bit j of byte k = qubit 8k + j), then eZ packed, then the ErrorCode flags byte.  Device
 * buffers, enqueued on `stream`. */
int qec_pack_decisions_dev(qec_decoder* dec, const uint8_t* eX, const uint8_t* eZ, const uint8_t* flags, size_t B,
                           uint8_t* out, void* stream);
/* A whole Monte-Carlo run on the device: `count` depolarising samples from `start` of stream
 * `seed`, in batches of `batch`: fused sample + syndrome -> packed decode (stop rule `stop`) ->
 * statistics with iteration sums, all on the device with no per-batch host synchronisation.
 * A multi-device decoder shards [start, start + count) contiguously over its parts.
 * Synchronous; fills *out (decodeSeconds: decode-kernel time, the largest over parts).
 * On a handle with priors: the samples of qec_sample_independent_dev, decoded with the priors, through the
 * unfused byte-syndrome pipeline; errorProbability is not used (qec_decoder_set_priors). */
int qec_monte_carlo(qec_decoder* dec, uint64_t seed, uint64_t start, uint64_t count, float errorProbability,
                    int maxIterations, int stop, size_t batch, qec_mc_result* out);

#ifdef __cplusplus
}
#endif
#endif /* QEC_LDPC_H */
