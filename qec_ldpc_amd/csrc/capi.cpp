// C ABI of libqecldpc.so (declared in include/qec_ldpc.h).
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>
#include <memory>
#include <new>
#include <stdexcept>
#include <algorithm>
#include <thread>

#include "../../include/HostDeviceArray.h"
#include "qec_internal.h"
#include "qec_near.h"
#include "qec_osd.h"

namespace {
// The handle's own events order work on one device (the workspace's cross-stream event) or time it
// (the Monte-Carlo ring); neither needs the system-scope release of a default event record (a cache
// writeback and invalidation between the launches around it; profiles/r06/ab/cmp_event_fence.txt).
constexpr unsigned kEvNoFence = hipEventDisableSystemFence;
}  // namespace

namespace qec {
const char* last_error_cstr();
const void* select_variant(const Code& c, std::string& name);
int launch_decode(const void* variant, const Code& c, const uint8_t* sX, const uint8_t* sZ, bool sbits, long long B,
                  float errorProbability, int maxIter, int stop, uint8_t* eX, uint8_t* eZ, uint8_t* flags,
                  uint8_t* rec, int32_t* iters, float* q, int hardPaths, const int32_t* perm, int split,
                  uint32_t* merge, bool merge_zeroed, hipStream_t stream, int rec_stride = 0, bool perm_sectors = false,
                  hipEvent_t done = nullptr, const uint16_t* memo = nullptr);
size_t memo_table_bytes(const void* variant, const Code& c);
size_t memo_workspace_bytes(const void* variant, const Code& c);
int launch_memo_fill(const void* variant, const Code& c, float errorProbability, int maxIter, int stop, int hardPaths,
                     uint16_t* table, uint8_t* ws, hipStream_t stream);
size_t schedule_workspace_bytes(long long B, int mX, int mZ);
bool schedule_sector_order(long long B, bool sbits, int mX, int mZ);
long long schedule_max_batch();
long long schedule_local_max_batch();
int launch_schedule(const uint8_t* sX, const uint8_t* sZ, bool sbits, long long B, int mX, int mZ, void* ws,
                    uint32_t* zero_merge, bool want_sectors, int32_t** perm_out, bool* sectors_out, hipStream_t st, int method, uint32_t* bar);
bool decode_uses_split(const void* variant, int stop, int split, long long B);
bool decode_needs_merge(const void* variant, int stop, int split, long long B);
int decode_sector_mode(const void* variant, int stop, int split, long long B, float p);
bool decode_has_list(const void* variant);
bool decode_pattern_masks(const void* variant, float errorProbability, uint32_t pats[4]);
int launch_decode_list(const void* variant, const Code& c, const uint8_t* sX, const uint8_t* sZ, long long B,
                       float errorProbability, int maxIter, int hardPaths, uint8_t* rec, int32_t* iters,
                       uint32_t* merge, const int32_t* listX, const int32_t* listZ, const uint32_t* counts,
                       hipStream_t stream, int rec_stride, bool merge_only, int count_stride, hipEvent_t done = nullptr);
bool triage_supported(const Code& c);
bool triage_aligned(const void* sX, const void* sZ);
int launch_triage(const Code& c, const uint32_t* sX, const uint32_t* sZ, long long B, const uint32_t pats[4],
                  uint8_t* rec, int32_t* iters, uint32_t* merge, int32_t* listX, int32_t* listZ, uint32_t* counts,
                  hipStream_t st, int rec_stride = 0);
bool decode_has_phase_stats(const void* variant, int stop);
int launch_sample_depolarizing(uint64_t seed, uint64_t start, long long B, int n, float p, uint8_t* x, uint8_t* z,
                               hipStream_t st);
int launch_mc_errors_syndrome(int src, const McArgsHost& h, hipStream_t st);
bool statistics_lane_shape(int estride, int rec_stride);
bool mc_fused_supported(const Code& c, int rec_stride);
int launch_mc_fused(const Code& c, uint64_t seed, uint64_t start, long long B, float p, const uint32_t pats[4],
                    uint32_t* sX, uint32_t* sZ, uint8_t* rec, int rec_stride, int32_t* iters, uint32_t* merge,
                    int32_t* listX, int32_t* listZ, int32_t* listS, uint32_t* counts, const uint64_t* imp_cols,
                    unsigned long long* counters, unsigned long long* partials, int stage, hipStream_t st);
long long mc_fused_parts(long long B);
int launch_zero_words(unsigned long long* w, int n, hipStream_t st, unsigned long long* w2 = nullptr, int n2 = 0);
int mc_fused_part_rows();
int mc_fused_count_words();
int mc_fused_count_stride();
// u64 words after the counters that hold the fused pipeline's list lengths
inline int mc_count_u64() { return (mc_fused_count_words() + 3) / 4 * 2; }  // whole 16-byte lines
int launch_statistics_packed(const Code& c, const uint64_t* imp_cols, const uint8_t* errp, int estride, const uint8_t* rec,
                             const int32_t* iters, long long B, unsigned long long* counters, hipStream_t st,
                             int rec_stride = 0);
int launch_logical_outcome(const Code& c, const uint64_t* imp_cols, const uint8_t* errp, const uint8_t* rec, long long B,
                           uint8_t* outcome, hipStream_t st);
void* sparse_plan_create(const Code& c, int device);
void sparse_plan_free(void* plan);
const char* sparse_plan_name(const void* plan);
const int32_t* sparse_plan_chkvar(const void* plan);
const int32_t* sparse_plan_varedge(const void* plan);
int launch_decode_sparse(void* plan, const SparseDecode& d, hipStream_t stream);
const void* select_wave_minsum(const Code& c);
std::string wave_minsum_name(const Code& c);
int launch_wave_minsum(const void* shape, const Code& c, const SparseDecode& d, hipStream_t stream);
// bp_wave_relay.hip
const void* select_wave_relay(const Code& c);
std::string wave_relay_name(const Code& c);
int launch_wave_relay(const void* shape, const Code& c, const SparseDecode& d, hipStream_t stream);
int launch_sample_pauli(uint64_t seed, uint64_t start, long long B, int n, const uint64_t* thr, uint8_t* x, uint8_t* z,
                        hipStream_t st);
int launch_sample_independent(uint64_t seed, uint64_t start, long long B, int n, const float* prior, uint8_t* x,
                              uint8_t* z, hipStream_t st);
void* cpu_plan_create(const Code& c);
void cpu_plan_free(void* plan);
int cpu_threads();
int cpu_decode_batch(void* plan, const uint8_t* sX, const uint8_t* sZ, long long B, float p, int maxIter, int stop,
                     uint8_t* eX, uint8_t* eZ, uint8_t* flags, uint8_t* rec, int32_t* iters, float* qf, int threads,
                     bool near_hard, const float* prior, int corr, const float* cond, int serial, int minsum,
                     const float* llr, const float* gamma, int legs, int solutions, const int32_t* weight, int layered,
                     const float* mu = nullptr, uint8_t* fX = nullptr, uint8_t* fZ = nullptr);
int launch_flip_syndrome(uint64_t seed, uint64_t start, long long B, int mX, int mZ, const float* q, uint8_t* sX,
                         uint8_t* sZ, uint8_t* fX, uint8_t* fZ, hipStream_t st);
int sparse_plan_relay_reserve(void* plan);
void correlated_priors(float p, float* c0, float* c1);
int launch_pack_decisions(const uint8_t* eX, const uint8_t* eZ, const uint8_t* flags, long long B, int n, uint8_t* out,
                          hipStream_t st);
int launch_statistics(const Code& c, const uint64_t* imp_cols, const uint8_t* x, const uint8_t* z, const uint8_t* eX,
                      const uint8_t* eZ, const uint8_t* flags, long long B, unsigned long long* counters, hipStream_t st);
struct OsdDevPlan;
std::string osd_dev_unsupported(const OsdPlan& P, int order, bool weighted);
OsdDevPlan* osd_dev_create(const OsdPlan& P);
void osd_dev_free(OsdDevPlan* D);
int launch_osd(const OsdDevPlan* D, int sweep, int order, const uint8_t* sX, const uint8_t* sZ, long long B, const float* q,
               uint8_t* eX, uint8_t* eZ, uint8_t* flags, uint32_t* repaired, uint32_t* swept, const int32_t* w,
               hipStream_t st, bool llr);
int launch_osd_collect(const uint8_t* rec, int rstride, int n, long long B, int32_t* list, uint32_t* count,
                       hipStream_t st);
int launch_osd_gather(const int32_t* list, long long cnt, const uint8_t* sX, const uint8_t* sZ, bool bits, int mX,
                      int mZ, const uint8_t* rec, int rstride, int n, uint8_t* oX, uint8_t* oZ, uint8_t* fl,
                      uint8_t* fl0, hipStream_t st);
int launch_osd_scatter(const int32_t* list, long long cnt, const uint8_t* eX, const uint8_t* eZ, const uint8_t* fl,
                       const uint8_t* fl0, int n, uint8_t* rec, int rstride, hipStream_t st);
}  // namespace qec

using namespace qec;

struct qec_code {
    Code c;
};


// One decoder handle: a device engine (wave-circulant variant or sparse-graph plan) plus the
// workspaces its entry points share, or a multi-device group of such handles (parts).
// Events owned by a handle (created on first use, destroyed with it on its device).
struct EventSet {
    std::vector<hipEvent_t> ev;
    ~EventSet()
    {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
    int make(size_t n, unsigned flags)
    {
        ev.assign(n, nullptr);
        for (auto& e : ev)
            if (hipEventCreateWithFlags(&e, flags) != hipSuccess) return qec::fail(QEC_ERR_HIP, "hipEventCreateWithFlags");
        return QEC_OK;
    }
};

struct qec_decoder {
    std::shared_ptr<const Code> code;
    int device = 0;
    int engine = QEC_ENGINE_CIRCULANT;
    const void* variant = nullptr;  // wave-circulant kernel variant (bp_decode.hip)
    void* sparse = nullptr;         // sparse-graph plan (bp_sparse.hip)
    void* cpu = nullptr;            // CPU engine plan (cpu_engine.cpp), device = -1
    std::string variant_name;
    int hard_paths = 1;             // QEC_OPT_HARD_PATHS
    int cycle_jump = 1;             // QEC_OPT_CYCLE_JUMP
    int near_hard = 1;              // QEC_OPT_NEAR_HARD_JUMP
    int near_probe = 1;             // QEC_OPT_NEAR_PROBE: the jump's division-free probe (bp_decode.hip, var_probe)
    // QEC_OPT_LIGHT_MEMO: sectors of one or two isolated qubit errors from a per-key outcome table (bp_decode.hip,
    // light_memo).  The table and the fill launch's workspace are allocated at creation (variants with the path);
    // memo_key = (bits of p', N, stop) of the table's content, filled on the stream of the first call with a new key
    int light_memo = 1;
    DeviceArray<uint16_t> memo_tab;
    DeviceArray<uint8_t> memo_ws;
    bool memo_valid = false;
    uint32_t memo_key[3] = {0, 0, 0};
    int schedule = 1;               // QEC_OPT_SCHEDULE (0 off, 1 auto, 2 always, 3 / 4 always, local / one-launch order)
    int sector_split = 1;           // QEC_OPT_SECTOR_SPLIT (0 off, 1 auto, 2 split waves, 3 sector launches)
    int phase_stats = 0;            // QEC_OPT_PHASE_STATS
    int triage = 1;                 // QEC_OPT_TRIAGE
    int last_path = 0;              // QEC_OPT_LAST_PATH: QEC_PATH_* bits of the last decode call
    int mc_time = 1;                // QEC_OPT_MC_DECODE_TIME
    int osd = 0;                    // QEC_OPT_OSD (0 off, 1 = OSD-0)
    int osd_iters = 3;              // QEC_OPT_OSD_ITERATIONS: iterations of the soft decode that feeds the order
    int osd_sweep = 0;              // QEC_OPT_OSD_SWEEP (0 per-chunk choice, 1 lanes across words, 2 lanes over rows)
    unsigned long long osd_sectors = 0;  // QEC_OPT_OSD_SECTORS: sectors repaired in the last call
    int osd_order = 0;              // QEC_OPT_OSD_ORDER: lambda of the combination sweep, 0 = OSD-0
    unsigned long long osd_cs_sectors = 0;  // QEC_OPT_OSD_CS_SECTORS: of those, the winner was not the OSD-0 estimate
    // per-qubit priors (qec_decoder_set_priors): the host copy (sector X [n], then Z [n]) and, on a GPU handle,
    // the device copy the PRIORS kernels and the independent sampler read (allocated on the first set,
    // rewritten in place afterwards); a group keeps the host copy and every part its own
    bool has_priors = false;
    std::vector<float> priors;
    DeviceArray<float> dpri;
    const float* prior_host() const { return has_priors ? priors.data() : nullptr; }
    const float* prior_dev() const { return has_priors ? dpri.data() : nullptr; }
    // QEC_OPT_CORRELATED ("The correlated form"): the option, and the second sector's
    // conditional priors c0_X [n], c1_X [n], c0_Z [n], c1_Z [n], kept beside the priors by every set (plain
    // priors: c0 = c1 = the marginal; a Pauli channel: its four tables); device copy as dpri
    int correlated = 0;
    int bp_schedule = 0;            // QEC_OPT_BP_SCHEDULE: 0 flooding, 1 the serial schedule
    // QEC_OPT_BP_METHOD (0 the product rule, 1 scaled min-sum; DESIGN.md section 2, "The min-sum form") and
    // QEC_OPT_MINSUM_SCALE (alpha = k / 256); the channel LLRs of the priors, sector X [n] then Z [n], built by every
    // set whatever the method says, as the OSD weight tables are; device copy as dpri
    int bp_method = 0;
    int minsum_scale = kMinSumDefaultScale;
    std::vector<float> mllr;
    DeviceArray<float> dmllr;
    int minsum() const { return bp_method == 1 ? minsum_scale : 0; }  // the engines' argument: 0, or the scale
    // QEC_OPT_MINSUM_WAVE: a sparse-engine handle's plain min-sum decodes run the wave kernels (bp_wave_minsum.hip);
    // data like minsum_scale, in effect while bp_method = 1 and no relay tables are set
    int minsum_wave = 0;
    // QEC_OPT_RELAY_WAVE: a sparse-engine handle's relay decodes run the wave kernels (bp_wave_relay.hip); data like
    // minsum_wave, in effect while bp_method = 1 and relay tables are set, whatever minsum_wave says
    int relay_wave = 0;
    // QEC_OPT_MINSUM_SCHEDULE: 0 flooding, 1 layered min-sum ("The layered min-sum form"); data like
    // minsum_scale, in effect while bp_method = 1 and no relay tables are set
    int minsum_schedule = 0;
    const float* llr_host() const { return has_priors ? mllr.data() : nullptr; }
    const float* llr_dev() const { return has_priors ? dmllr.data() : nullptr; }
    // qec_decoder_set_relay ("The relay form"): L legs of per-variable memory strengths, [leg][sector][n],
    // and S = the solutions to collect; data like minsum_scale, in effect while bp_method = 1.  The device copy is
    // allocated once, by the first set, at the largest legal size (2 * 2^22 floats), and rewritten in place afterwards,
    // so that no later set moves it under a captured graph; the kernels' workspace is allocated with it (the plan).
    // relay_hold: the OSD stage's soft decode runs without the tables.
    int relay_legs = 0, relay_solutions = 0;
    bool relay_hold = false;
    std::vector<float> relay;
    DeviceArray<float> drelay;
    bool relay_on() const { return relay_legs > 0 && bp_method == 1 && !relay_hold; }
    const float* relay_host() const { return relay_on() ? relay.data() : nullptr; }
    const float* relay_dev() const { return relay_on() ? drelay.data() : nullptr; }
    bool layered_on() const { return bp_method == 1 && minsum_schedule == 1 && !relay_on(); }
    // the weights of a relay solution: the integer tables of the priors (as qec_decoder_get_osd_weights), or none
    const int32_t* relay_w_host() const { return has_priors ? osw.data() : nullptr; }
    const int32_t* relay_w_dev() const { return has_priors ? dosw.data() : nullptr; }
    // qec_decoder_set_syndrome_priors ("The soft-syndrome form"): the probability that each check's
    // measured bit is flipped, sector X [mX] then Z [mZ], and their channel LLRs mu; the device copy (the LLRs, then the
    // priors for the flip sampler) is allocated by the first set and rewritten in place afterwards, as dpri is.  Set only
    // while bp_method = 1 and no relay tables are set (the calls refuse each other), so every min-sum decode of the
    // handle then runs under them.
    bool has_syn = false;
    std::vector<float> synq, synmu;
    DeviceArray<float> dsyn;
    bool soft_on() const { return has_syn && bp_method == 1 && !relay_on(); }
    const float* mu_host() const { return soft_on() ? synmu.data() : nullptr; }
    const float* mu_dev() const { return soft_on() ? dsyn.data() : nullptr; }
    const float* synq_dev() const { return dsyn.data() + synq.size(); }
    DeviceArray<uint8_t> fX, fZ;    // staging of the measurement decisions for qec_decode_batch_soft
    std::vector<float> cond;
    DeviceArray<float> dcond;
    const float* cond_host() const { return has_priors ? cond.data() : nullptr; }
    const float* cond_dev() const { return has_priors ? dcond.data() : nullptr; }
    // Per-qubit Pauli channel (qec_decoder_set_pauli_channel): pX [n], pY [n], pZ [n] and the sampler's 64-bit
    // thresholds tX [n], tXY [n], tXYZ [n] (device copy as dpri)
    bool has_channel = false;
    std::vector<float> pauli;
    DeviceArray<uint64_t> dpth;
    // QEC_OPT_OSD_SCORE: the rule, and the sweep's weight tables (sector X [n], then Z [n]), rebuilt by
    // every qec_decoder_set_priors; the device copy is allocated and rewritten as dpri is.  The sweep takes
    // the tables only with the rule at 1 and priors set (else the pointers are null: Hamming weight)
    int osd_score = 0;
    std::vector<int32_t> osw;
    DeviceArray<int32_t> dosw;
    bool osd_weighted() const { return osd_score == 1 && has_priors; }
    const int32_t* osw_host() const { return osd_weighted() ? osw.data() : nullptr; }
    const int32_t* osw_dev() const { return osd_weighted() ? dosw.data() : nullptr; }
    // OSD stage: the elimination tables (host; device copy for the GPU engines), the compact
    // batch of failed samples (syndromes, estimates, flags, soft output) and the failed-record list
    std::shared_ptr<const OsdPlan> oplan;
    OsdDevPlan* odev = nullptr;
    std::string osd_why;            // why the kernel cannot take this code (empty: it can)
    DeviceArray<uint8_t> osX, osZ, oeX, oeZ, ofl, ofl0, ofs;
    DeviceArray<float> oq;
    DeviceArray<int32_t> olist;
    DeviceArray<uint32_t> ocnt;     // [0] list length, [1] sectors repaired, [2] of those swept (index > 0)
    PinnedArray<uint32_t> ocnt_h;
    // workspace shared by every launch of this handle (dispatch order, split-flag merge words,
    // sparse byte staging for packed output); ws_ev marks the last launch that used it, so a call
    // on another stream waits for it (stream-ordered reuse)
    DeviceArray<uint8_t> sched;
    DeviceArray<uint32_t> merge;
    DeviceArray<uint32_t> gbar;  // grid-barrier words of the one-launch dispatch order (zeroed at creation)
    DeviceArray<int32_t> tlist;  // triage: listX [B], listZ [B], (fused Monte-Carlo: listS [B]), counts
    hipEvent_t ws_ev = nullptr;
    hipStream_t ws_stream = nullptr;
    bool ws_used = false;
    hipStream_t stream = nullptr;   // the host-pointer and Monte-Carlo entry points' stream
    // staging for the host-pointer entry points (DecoderGPU's device vectors, DecoderGPU.h:28-35)
    DeviceArray<uint8_t> sX, sZ, eX, eZ, flags, rec;
    DeviceArray<int32_t> iters;
    DeviceArray<float> q;
    // Monte-Carlo workspace (qec_monte_carlo / qec_get_statistics)
    DeviceArray<uint64_t> imp_cols;  // I-P by columns over its non-zero rows (Code::imp_cols)
    DeviceArray<uint8_t> msX, msZ, merrp, mrec, mtype;
    DeviceArray<int32_t> mit, midx;
    DeviceArray<unsigned long long> mcount;
    DeviceArray<unsigned long long> mpart;  // fused Monte-Carlo kernel: partial-sum rows of the counters
    PinnedArray<unsigned long long> mhost;  // the counters' host copy (page-locked: an asynchronous copy)
    EventSet mc_ev;  // qec_monte_carlo's ring of decode-time event pairs
    // multi-device group (qec_decoder_create_multi): the parts do the work, this handle only routes
    std::vector<qec_decoder*> parts;

    ~qec_decoder()
    {
        for (qec_decoder* p : parts) delete p;
        if (cpu) cpu_plan_free(cpu);
        if (parts.empty() && !cpu) {
            // the member device arrays are freed after this body, on this device too;
            // qec_decoder_destroy restores the caller's device afterwards
            (void)hipSetDevice(device);
            if (ws_ev) (void)hipEventDestroy(ws_ev);
            if (stream) (void)hipStreamDestroy(stream);
            if (sparse) sparse_plan_free(sparse);
            if (odev) osd_dev_free(odev);
        }
    }
};

#define QEC_HIP_CHECK(expr)                                                                     \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) return fail(QEC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

namespace {

// Makes `device` current for the scope of an entry point and restores the caller's device.
struct DeviceGuard {
    int prev = -1;
    hipError_t err;
    explicit DeviceGuard(int device)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        err = hipSetDevice(device);
    }
    ~DeviceGuard()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

#define QEC_DEVICE_SCOPE(dev)                                                                      \
    DeviceGuard guard_(dev);                                                                       \
    if (guard_.err != hipSuccess) return fail(QEC_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(guard_.err))

bool capturing(hipStream_t st)
{
    hipStreamCaptureStatus s = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(st, &s) == hipSuccess && s != hipStreamCaptureStatusNone;
}

// Grow a workspace buffer to n elements.  Refused while `st` is being captured into a graph (an
// allocation there would be invalid): size the decoder with max_batch instead.
template <class T>
int ws_reserve(DeviceArray<T>& a, size_t n, hipStream_t st, const char* what)
{
    if (n <= a.capacity()) return QEC_OK;
    if (capturing(st))
        return fail(QEC_ERR_ARG, std::string(what) + ": the workspace is smaller than this batch and the stream is "
                                                     "being captured; create the decoder with max_batch >= B");
    try {
        a.reserve(n);
    } catch (const std::exception& ex) {
        return fail(QEC_ERR_NOMEM, std::string(what) + ": " + ex.what());
    }
    return QEC_OK;
}

// Stream-ordered use of the handle's workspace: a launch on a stream other than the previous
// one first waits for the previous launch's completion event.  Launches captured into a graph
// neither wait nor record (an event outside the capture cannot be waited on inside it): the
// graph's replays are ordered by its launcher.
int ws_acquire(qec_decoder* d, hipStream_t st)
{
    if (d->ws_used && st != d->ws_stream && !capturing(st)) QEC_HIP_CHECK(hipStreamWaitEvent(st, d->ws_ev, 0));
    return QEC_OK;
}
// The workspace event for the call's last kernel to carry (launch_marked), or null while capturing;
// ws_release(d, st, true) then records nothing more.
hipEvent_t ws_done(qec_decoder* d, hipStream_t st) { return capturing(st) ? nullptr : d->ws_ev; }
int ws_release(qec_decoder* d, hipStream_t st, bool carried = false)
{
    if (capturing(st)) return QEC_OK;
    if (!carried) QEC_HIP_CHECK(hipEventRecord(d->ws_ev, st));
    d->ws_used = true;
    d->ws_stream = st;
    return QEC_OK;
}

std::vector<qec_decoder*> parts_of(qec_decoder* d)
{
    if (d->parts.empty()) return {d};
    return d->parts;
}

// contiguous shard k of n over [0, B): [k B / n, (k + 1) B / n)
long long shard_lo(long long B, int k, int n) { return (long long)((__int128)B * k / n); }

}  // namespace

extern "C" {

const char* qec_last_error(void) { return last_error_cstr(); }
int qec_abi_version(void) { return QEC_LDPC_ABI_VERSION; }
#ifndef QEC_BUILD_ID
#define QEC_BUILD_ID "unknown"
#endif
const char* qec_build_id(void) { return QEC_BUILD_ID; }

qec_code* qec_code_load(const char* path)
{
    if (!path) { fail(QEC_ERR_ARG, "qec_code_load: null path"); return nullptr; }
    auto* h = new (std::nothrow) qec_code;
    if (!h) { fail(QEC_ERR_NOMEM, "qec_code_load: out of memory"); return nullptr; }
    if (load_code(path, h->c) != QEC_OK) { delete h; return nullptr; }
    return h;
}

qec_code* qec_code_generate(int J, int K, int L, int P, int sigma, int tau)
{
    auto* h = new (std::nothrow) qec_code;
    if (!h) { fail(QEC_ERR_NOMEM, "qec_code_generate: out of memory"); return nullptr; }
    if (generate_code(J, K, L, P, sigma, tau, h->c) != QEC_OK) { delete h; return nullptr; }
    return h;
}

qec_code* qec_code_from_matrices(int n, int mX, const uint8_t* HX, int mZ, const uint8_t* HZ)
{
    auto* h = new (std::nothrow) qec_code;
    if (!h) { fail(QEC_ERR_NOMEM, "qec_code_from_matrices: out of memory"); return nullptr; }
    try {
        if (general_code(n, mX, HX, mZ, HZ, nullptr, h->c) != QEC_OK) { delete h; return nullptr; }
    } catch (const std::bad_alloc&) {
        delete h;
        fail(QEC_ERR_NOMEM, "qec_code_from_matrices: out of memory");
        return nullptr;
    }
    return h;
}

int qec_code_degrees(const qec_code* h, int* out)
{
    if (!h || !out) return fail(QEC_ERR_ARG, "qec_code_degrees: null argument");
    code_degrees(h->c, out);
    return QEC_OK;
}

int qec_code_has_wave_minsum(const qec_code* h)
{
    if (!h) return fail(QEC_ERR_ARG, "qec_code_has_wave_minsum: null code");
    return select_wave_minsum(h->c) != nullptr ? 1 : 0;
}

int qec_code_layers(const qec_code* h, int sector, int32_t* colour)
{
    if (!h || (sector != 0 && sector != 1)) return fail(QEC_ERR_ARG, "qec_code_layers: bad argument");
    return code_layers(h->c, sector, colour);
}

int qec_code_free(qec_code* code)
{
    delete code;
    return QEC_OK;
}

int qec_code_params(const qec_code* h, int* out)
{
    if (!h || !out) return fail(QEC_ERR_ARG, "qec_code_params: null argument");
    const Code& c = h->c;
    const int v[9] = {c.J, c.K, c.L, c.P, c.sigma, c.tau, c.n, c.mX, c.mZ};
    std::memcpy(out, v, sizeof v);
    return QEC_OK;
}

int qec_code_exponents(const qec_code* h, int sector, int* out)
{
    if (!h || !out || (sector != 0 && sector != 1)) return fail(QEC_ERR_ARG, "qec_code_exponents: bad argument");
    if (!h->c.is_qc) return fail(QEC_ERR_UNSUPPORTED, "code is not built from circulant permutation blocks");
    const std::vector<int>& E = sector ? h->c.EZ : h->c.EX;
    std::memcpy(out, E.data(), E.size() * sizeof(int));
    return QEC_OK;
}

int qec_code_pcm(const qec_code* h, int sector, uint8_t* out)
{
    if (!h || !out || (sector != 0 && sector != 1)) return fail(QEC_ERR_ARG, "qec_code_pcm: bad argument");
    const std::vector<uint8_t>& H = sector ? h->c.pcmZ : h->c.pcmX;
    std::memcpy(out, H.data(), H.size());
    return QEC_OK;
}

int qec_code_describe(const qec_code* h, char* buf, size_t len)
{
    if (!h || !buf || !len) return fail(QEC_ERR_ARG, "qec_code_describe: bad argument");
    const std::string s = h->c.describe();
    std::snprintf(buf, len, "%s", s.c_str());
    return QEC_OK;
}

int qec_code_syndrome(const qec_code* h, int sector, const uint8_t* e, size_t B, uint8_t* s)
{
    if (!h || (B && (!e || !s)) || (sector != 0 && sector != 1)) return fail(QEC_ERR_ARG, "qec_code_syndrome: bad argument");
    const Code& c = h->c;
    const int m = sector ? c.mZ : c.mX;
    for (size_t b = 0; b < B; ++b) host_syndrome(c, sector, e + b * c.n, s + b * m);
    return QEC_OK;
}

int qec_code_check_logical(const qec_code* h, const uint8_t* ex, const uint8_t* ez, size_t B, uint8_t* out)
{
    if (!h || (B && (!ex || !ez || !out))) return fail(QEC_ERR_ARG, "qec_code_check_logical: bad argument");
    if (h->c.imp.empty()) return fail(QEC_ERR_UNSUPPORTED, "code has no I-P matrix (generated codes carry none)");
    for (size_t b = 0; b < B; ++b) out[b] = host_check_logical(h->c, ex + b * h->c.n, ez + b * h->c.n) ? 1 : 0;
    return QEC_OK;
}

qec_code* qec_code_with_logical(const qec_code* code, int mode)
{
    if (!code) { fail(QEC_ERR_ARG, "qec_code_with_logical: null code"); return nullptr; }
    auto* h = new (std::nothrow) qec_code;
    if (!h) { fail(QEC_ERR_NOMEM, "qec_code_with_logical: out of memory"); return nullptr; }
    try {
        if (derive_logical(code->c, mode, h->c) != QEC_OK) { delete h; return nullptr; }
    } catch (const std::bad_alloc&) {
        delete h;
        fail(QEC_ERR_NOMEM, "qec_code_with_logical: out of memory");
        return nullptr;
    }
    return h;
}

int qec_code_logical_mode(const qec_code* code)
{
    if (!code) return fail(QEC_ERR_ARG, "qec_code_logical_mode: null code");
    return code->c.logical_mode;
}

int qec_code_logical_rows(const qec_code* code, int* rows)
{
    if (!code || !rows) return fail(QEC_ERR_ARG, "qec_code_logical_rows: null argument");
    *rows = code->c.imp_words ? (int)(code->c.imp_rows.size() / code->c.imp_words) : 0;
    return QEC_OK;
}

int qec_code_imp(const qec_code* code, uint8_t* out)
{
    if (!code || !out) return fail(QEC_ERR_ARG, "qec_code_imp: null argument");
    if (code->c.imp.empty()) return fail(QEC_ERR_UNSUPPORTED, "code has no I-P matrix (qec_code_with_logical derives one)");
    std::memcpy(out, code->c.imp.data(), code->c.imp.size());
    return QEC_OK;
}


qec_decoder* qec_decoder_create(const qec_code* h, int device, size_t max_batch)
{
    return qec_decoder_create_engine(h, device, max_batch, QEC_ENGINE_AUTO);
}

qec_decoder* qec_decoder_create_engine(const qec_code* h, int device, size_t max_batch, int engine)
{
    if (!h) { fail(QEC_ERR_ARG, "qec_decoder_create: null code"); return nullptr; }
    if (engine < QEC_ENGINE_AUTO || engine > QEC_ENGINE_CPU) {
        fail(QEC_ERR_ARG, "qec_decoder_create_engine: unknown engine");
        return nullptr;
    }
    if (device < 0 || engine == QEC_ENGINE_CPU) {  // DecoderCPU: host buffers only
        if (device >= 0 || (engine != QEC_ENGINE_AUTO && engine != QEC_ENGINE_CPU)) {
            fail(QEC_ERR_ARG, "qec_decoder_create: the CPU engine is device -1, the GPU engines devices >= 0");
            return nullptr;
        }
        std::unique_ptr<qec_decoder> d(new (std::nothrow) qec_decoder);
        if (!d) { fail(QEC_ERR_NOMEM, "qec_decoder_create: out of memory"); return nullptr; }
        d->code = std::make_shared<const Code>(h->c);
        d->device = -1;
        d->engine = QEC_ENGINE_CPU;
        d->cpu = cpu_plan_create(*d->code);
        if (!d->cpu) return nullptr;
        {
            auto op = std::make_shared<OsdPlan>();
            osd_plan_build(*d->code, *op);
            d->oplan = op;
        }
        d->variant_name = "cpu (" + std::to_string(cpu_threads()) + " threads) " + d->code->describe();
        return d.release();
    }
    std::string name;
    const void* v = engine == QEC_ENGINE_SPARSE || h->c.general ? nullptr : select_variant(h->c, name);
    if (!v && engine == QEC_ENGINE_CIRCULANT) {
        fail(QEC_ERR_UNSUPPORTED, "no wave-circulant kernel for this code shape (" + h->c.describe() +
                                      "): needs circulant-permutation blocks, P <= 64 and an instantiated (J,K,L)");
        return nullptr;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        fail(QEC_ERR_HIP, "qec_decoder_create: no HIP device available");
        return nullptr;
    }
    if (device >= ndev) { fail(QEC_ERR_ARG, "qec_decoder_create: device ordinal out of range"); return nullptr; }
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) { fail(QEC_ERR_HIP, "hipSetDevice failed"); return nullptr; }
    std::unique_ptr<qec_decoder> d(new (std::nothrow) qec_decoder);
    if (!d) { fail(QEC_ERR_NOMEM, "qec_decoder_create: out of memory"); return nullptr; }
    d->code = std::make_shared<const Code>(h->c);
    d->device = device;
    d->variant = v;
    d->variant_name = name;
    if (!v) {  // AUTO without a wave-circulant kernel, or SPARSE requested
        d->engine = QEC_ENGINE_SPARSE;
        d->sparse = sparse_plan_create(*d->code, device);
        if (!d->sparse) return nullptr;  // error text set by the plan
        d->variant_name = sparse_plan_name(d->sparse);
    }
    if (hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&d->ws_ev, hipEventDisableTiming | kEvNoFence) != hipSuccess) {
        fail(QEC_ERR_HIP, "qec_decoder_create: stream / event creation failed");
        return nullptr;
    }
    try {
        // the device-pointer workspace is sized up front so that the _dev entry points allocate
        // nothing for batches up to max_batch (graph capture); staging grows on demand
        if (max_batch > 0 && d->variant) {
            if ((long long)max_batch <= schedule_max_batch())
                d->sched.reserve(schedule_workspace_bytes((long long)max_batch, d->code->mX, d->code->mZ));
            d->merge.reserve(max_batch);
        }
        if (max_batch > 0 && d->sparse) {
            d->eX.reserve(max_batch * d->code->n);
            d->eZ.reserve(max_batch * d->code->n);
            d->flags.reserve(max_batch);
        }
        if (!d->code->imp_cols.empty()) {
            d->imp_cols.reserve(d->code->imp_cols.size());
            hip_throw(hipMemcpy(d->imp_cols.data(), d->code->imp_cols.data(), d->code->imp_cols.size() * sizeof(uint64_t),
                                hipMemcpyHostToDevice), "I-P upload");
        }
        // the counters, then the fused pipeline's list lengths: one memset zeroes both per call
        d->mcount.reserve(QEC_MC_NCOUNTERS_ALL + mc_count_u64());
        if (d->variant && memo_table_bytes(d->variant, *d->code)) {
            d->memo_tab.reserve(memo_table_bytes(d->variant, *d->code) / sizeof(uint16_t));
            d->memo_ws.reserve(memo_workspace_bytes(d->variant, *d->code));
        }
        if (d->variant) {
            d->gbar.reserve(2);
            hip_throw(hipMemset(d->gbar.data(), 0, 2 * sizeof(uint32_t)), "grid-barrier words");
        }
        // the OSD stage's tables (a code the kernel cannot take keeps the reason for the OSD entry points)
        auto op = std::make_shared<OsdPlan>();
        osd_plan_build(*d->code, *op);
        d->oplan = op;
        d->osd_why = osd_dev_unsupported(*op, 0, false);
        if (d->osd_why.empty()) {
            d->odev = osd_dev_create(*op);
            if (!d->odev) return nullptr;
            d->ocnt.reserve(3);
            hip_throw(hipMemset(d->ocnt.data(), 0, 3 * sizeof(uint32_t)), "OSD counters");
        }
    } catch (const std::exception& ex) {
        fail(QEC_ERR_HIP, std::string("qec_decoder_create: ") + ex.what());
        return nullptr;
    }
    return d.release();
}

qec_decoder* qec_decoder_create_multi(const qec_code* h, const int* devices, int ndevices, size_t max_batch)
{
    return qec_decoder_create_multi_engine(h, devices, ndevices, max_batch, QEC_ENGINE_AUTO);
}

qec_decoder* qec_decoder_create_multi_engine(const qec_code* h, const int* devices, int ndevices, size_t max_batch,
                                             int engine)
{
    if (engine == QEC_ENGINE_CPU) {
        fail(QEC_ERR_ARG, "qec_decoder_create_multi_engine: a group is GPU-only (QEC_ENGINE_AUTO, _CIRCULANT or _SPARSE)");
        return nullptr;
    }
    if (!h || !devices || ndevices <= 0) { fail(QEC_ERR_ARG, "qec_decoder_create_multi: bad argument"); return nullptr; }
    for (int k = 0; k < ndevices; ++k)
        if (devices[k] < 0) {
            // a CPU-engine part would decode host batches but fail the device-side entry points
            // (statistics, Monte-Carlo) of the group: groups are GPU-only
            fail(QEC_ERR_ARG, "qec_decoder_create_multi: device ordinals must be >= 0 (the CPU engine is device -1 of "
                              "qec_decoder_create)");
            return nullptr;
        }
    std::unique_ptr<qec_decoder> g(new (std::nothrow) qec_decoder);
    if (!g) { fail(QEC_ERR_NOMEM, "qec_decoder_create_multi: out of memory"); return nullptr; }
    for (int k = 0; k < ndevices; ++k) {
        qec_decoder* p = qec_decoder_create_engine(h, devices[k], max_batch, engine);
        if (!p) return nullptr;  // parts created so far are freed with g
        g->parts.push_back(p);
    }
    const qec_decoder* p0 = g->parts[0];
    g->code = p0->code;
    g->device = p0->device;
    g->engine = p0->engine;
    g->variant = p0->variant;
    std::string name = "multi-device [";
    for (int k = 0; k < ndevices; ++k) name += (k ? "," : "") + std::to_string(devices[k]);
    g->variant_name = name + "] " + p0->variant_name;
    return g.release();
}

int qec_decoder_num_parts(const qec_decoder* d)
{
    if (!d) return fail(QEC_ERR_ARG, "qec_decoder_num_parts: null decoder");
    return d->parts.empty() ? 1 : (int)d->parts.size();
}

qec_decoder* qec_decoder_part(qec_decoder* d, int k)
{
    if (!d) { fail(QEC_ERR_ARG, "qec_decoder_part: null decoder"); return nullptr; }
    if (d->parts.empty()) return k == 0 ? d : (fail(QEC_ERR_ARG, "qec_decoder_part: index out of range"), nullptr);
    if (k < 0 || k >= (int)d->parts.size()) { fail(QEC_ERR_ARG, "qec_decoder_part: index out of range"); return nullptr; }
    return d->parts[k];
}

int qec_decoder_device(const qec_decoder* d)
{
    if (!d) return fail(QEC_ERR_ARG, "qec_decoder_device: null decoder");
    return d->device;
}

int qec_decoder_destroy(qec_decoder* d)
{
    // every part's streams, events and device arrays are freed on its own device; the caller's
    // current device is restored afterwards (as every other entry point does)
    int prev = -1;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    delete d;
    if (prev >= 0) (void)hipSetDevice(prev);
    return QEC_OK;
}

int qec_decoder_describe(const qec_decoder* d, char* buf, size_t len)
{
    if (!d || !buf || !len) return fail(QEC_ERR_ARG, "qec_decoder_describe: bad argument");
    std::string text = d->variant_name;
    if (d->minsum_wave)  // the kernels of the handle's plain min-sum decodes
        text += " [min-sum: " + wave_minsum_name(*d->code) + "]";
    if (d->relay_wave)   // ... and of its relay decodes
        text += " [relay: " + wave_relay_name(*d->code) + "]";
    if (d->has_syn) text += " [soft syndrome]";
    std::snprintf(buf, len, "%s", text.c_str());
    return QEC_OK;
}

int qec_near_hard_threshold(float pPrime, int R, int L, float* eps0, uint32_t* T)
{
    if (!eps0 || !T) return fail(QEC_ERR_ARG, "qec_near_hard_threshold: bad argument");
    const NearHard t = near_hard_threshold(pPrime, R, L);
    *eps0 = t.eps0;
    *T = t.T;
    return QEC_OK;
}

int qec_near_probe(float t0, float t1, float eps0, int* side)
{
    int s = 0;
    const bool ok = near_probe(t0, t1, eps0, s);
    if (side) *side = s;
    return ok ? 1 : 0;
}

// QEC_OPT_MINSUM_WAVE and QEC_OPT_RELAY_WAVE (`name`): 0 or 1 into `field`; 1 on a single handle needs the sparse engine
// and a code with wave kernels (`select`).  `what` names the rule ("min-sum", "relay"), `alone` what only the sparse
// engine does with it.
static int set_wave_option(qec_decoder* d, int value, int& field, const std::string& name, const char* what,
                           const char* alone, const void* (*select)(const Code&))
{
    const std::string who = "qec_decoder_set_option: " + name;
    if (value != 0 && value != 1) return fail(QEC_ERR_ARG, who + " is 0 (the sparse-graph kernels) or 1 (the wave kernels)");
    if (value && d->parts.empty()) {
        if (d->cpu)
            return fail(QEC_ERR_UNSUPPORTED,
                        who + " = 1 chooses GPU kernels; the CPU engine has one " + what + " implementation");
        if (d->engine != QEC_ENGINE_SPARSE)
            return fail(QEC_ERR_UNSUPPORTED,
                        who + " = 1 is a kernel choice of a sparse-engine handle, which alone " + alone +
                            "; create the decoder with QEC_ENGINE_SPARSE (engine \"sparse\")");
        if (!select(*d->code))
            return fail(QEC_ERR_UNSUPPORTED,
                        who + " = 1: no wave " + what + " kernel for this code (" + d->code->describe() +
                            "): needs circulant-permutation blocks, P <= 64 and a block shape (J,K,L) of the "
                            "runtime-shift table");
    }
    field = value;
    return QEC_OK;
}

int qec_decoder_set_option(qec_decoder* d, int option, int value)
{
    if (!d) return fail(QEC_ERR_ARG, "qec_decoder_set_option: null decoder");
    for (qec_decoder* p : d->parts) {
        const int rc = qec_decoder_set_option(p, option, value);
        if (rc) return rc;
    }
    switch (option) {
    case QEC_OPT_HARD_PATHS: d->hard_paths = value != 0; return QEC_OK;
    case QEC_OPT_CYCLE_JUMP: d->cycle_jump = value != 0; return QEC_OK;
    case QEC_OPT_NEAR_HARD_JUMP: d->near_hard = value != 0; return QEC_OK;
    case QEC_OPT_NEAR_PROBE: d->near_probe = value != 0; return QEC_OK;
    case QEC_OPT_LIGHT_MEMO: d->light_memo = value != 0; return QEC_OK;
    case QEC_OPT_SCHEDULE:
        if (value < 0 || value > 4) return fail(QEC_ERR_ARG, "qec_decoder_set_option: QEC_OPT_SCHEDULE is 0 .. 4");
        d->schedule = value;
        return QEC_OK;
    case QEC_OPT_SECTOR_SPLIT:
        if (value < 0 || value > 3) return fail(QEC_ERR_ARG, "qec_decoder_set_option: QEC_OPT_SECTOR_SPLIT is 0 .. 3");
        d->sector_split = value;
        return QEC_OK;
    case QEC_OPT_PHASE_STATS:
        if (value && (!d->variant || !decode_has_phase_stats(d->variant, QEC_STOP_FIXED)))
            return fail(QEC_ERR_UNSUPPORTED, "qec_decoder_set_option: QEC_OPT_PHASE_STATS needs a shipped code's kernels");
        d->phase_stats = value != 0;
        return QEC_OK;
    case QEC_OPT_TRIAGE:
        if (value < 0 || value > 3) return fail(QEC_ERR_ARG, "qec_decoder_set_option: QEC_OPT_TRIAGE is 0 .. 3");
        d->triage = value;
        return QEC_OK;
    case QEC_OPT_MC_DECODE_TIME: d->mc_time = value != 0; return QEC_OK;
    case QEC_OPT_OSD:
        if (value != 0 && value != 1) return fail(QEC_ERR_ARG, "qec_decoder_set_option: QEC_OPT_OSD is 0 (off) or 1 (OSD-0)");
        if (value && d->parts.empty() && !d->cpu && !d->odev) return fail(QEC_ERR_UNSUPPORTED, d->osd_why);
        if (value && d->has_syn)
            return fail(QEC_ERR_UNSUPPORTED,
                        "qec_decoder_set_option: QEC_OPT_OSD = 1 solves H e = s exactly, which is not the problem under "
                        "syndrome priors; clear them (qec_decoder_set_syndrome_priors(dec, NULL, NULL)) first");
        d->osd = value;
        return QEC_OK;
    case QEC_OPT_OSD_ITERATIONS:
        if (value < 1) return fail(QEC_ERR_ARG, "qec_decoder_set_option: QEC_OPT_OSD_ITERATIONS is >= 1");
        d->osd_iters = value;
        return QEC_OK;
    case QEC_OPT_OSD_SECTORS: return fail(QEC_ERR_ARG, "qec_decoder_set_option: QEC_OPT_OSD_SECTORS is read only");
    case QEC_OPT_OSD_SWEEP:
        if (value < 0 || value > 2) return fail(QEC_ERR_ARG, "qec_decoder_set_option: QEC_OPT_OSD_SWEEP is 0 .. 2");
        d->osd_sweep = value;
        return QEC_OK;
    case QEC_OPT_OSD_ORDER:
        if (value < 0 || value > kOsdMaxOrder) return fail(QEC_ERR_ARG, "qec_decoder_set_option: QEC_OPT_OSD_ORDER is 0 .. 64");
        if (value && d->odev) {  // the sweep's column vectors share the workgroup's LDS with [H | s]
            const std::string why = osd_dev_unsupported(*d->oplan, value, d->osd_weighted());
            if (!why.empty()) return fail(QEC_ERR_UNSUPPORTED, why);
        }
        d->osd_order = value;
        return QEC_OK;
    case QEC_OPT_OSD_SCORE:
        if (value != 0 && value != 1)
            return fail(QEC_ERR_ARG, "qec_decoder_set_option: QEC_OPT_OSD_SCORE is 0 (Hamming weight) or 1 (prior-weighted)");
        if (value && d->odev && d->has_priors && d->osd_order > 0) {  // the weighted sweep's arrays need LDS of their own
            const std::string why = osd_dev_unsupported(*d->oplan, d->osd_order, true);
            if (!why.empty()) return fail(QEC_ERR_UNSUPPORTED, why);
        }
        d->osd_score = value;
        return QEC_OK;
    case QEC_OPT_CORRELATED:
        if (value < 0 || value > 2)
            return fail(QEC_ERR_ARG, "qec_decoder_set_option: QEC_OPT_CORRELATED is 0 (off), 1 (X first) or 2 (Z first)");
        if (value && d->parts.empty() && !d->cpu && d->engine != QEC_ENGINE_SPARSE)
            return fail(QEC_ERR_UNSUPPORTED,
                        "qec_decoder_set_option: QEC_OPT_CORRELATED needs per-sample priors, which the wave-circulant engine "
                        "cannot hold; create the decoder with QEC_ENGINE_SPARSE (engine \"sparse\")");
        if (value && d->bp_schedule)
            return fail(QEC_ERR_UNSUPPORTED,
                        "qec_decoder_set_option: QEC_OPT_CORRELATED has no form under the serial schedule; set "
                        "QEC_OPT_BP_SCHEDULE to 0 (flooding) first");
        if (value && d->bp_method)
            return fail(QEC_ERR_UNSUPPORTED,
                        "qec_decoder_set_option: QEC_OPT_CORRELATED has no min-sum form; set QEC_OPT_BP_METHOD to 0 (the "
                        "product rule) first");
        d->correlated = value;
        return QEC_OK;
    case QEC_OPT_BP_SCHEDULE:
        if (value != 0 && value != 1)
            return fail(QEC_ERR_ARG, "qec_decoder_set_option: QEC_OPT_BP_SCHEDULE is 0 (flooding) or 1 (serial)");
        if (value && d->parts.empty() && !d->cpu && d->engine != QEC_ENGINE_SPARSE)
            return fail(QEC_ERR_UNSUPPORTED,
                        "qec_decoder_set_option: QEC_OPT_BP_SCHEDULE = 1 (serial) is not built for the wave-circulant engine, "
                        "whose hard-message shortcuts are proven for flooding; create the decoder with QEC_ENGINE_SPARSE "
                        "(engine \"sparse\")");
        if (value && d->correlated)
            return fail(QEC_ERR_UNSUPPORTED,
                        "qec_decoder_set_option: the serial schedule has no correlated form; set QEC_OPT_CORRELATED to 0 "
                        "first");
        if (value && d->bp_method)
            return fail(QEC_ERR_UNSUPPORTED,
                        "qec_decoder_set_option: min-sum is built for the flooding schedule; set QEC_OPT_BP_METHOD to 0 (the "
                        "product rule) first");
        d->bp_schedule = value;
        return QEC_OK;
    case QEC_OPT_BP_METHOD:
        if (value != 0 && value != 1)
            return fail(QEC_ERR_ARG, "qec_decoder_set_option: QEC_OPT_BP_METHOD is 0 (the product rule) or 1 (scaled min-sum)");
        if (value && d->parts.empty() && !d->cpu && d->engine != QEC_ENGINE_SPARSE)
            return fail(QEC_ERR_UNSUPPORTED,
                        "qec_decoder_set_option: QEC_OPT_BP_METHOD = 1 (min-sum) is not built for the wave-circulant engine, "
                        "whose kernels and hard-message shortcuts are the product rule's; create the decoder with "
                        "QEC_ENGINE_SPARSE (engine \"sparse\")");
        if (value && d->correlated)
            return fail(QEC_ERR_UNSUPPORTED,
                        "qec_decoder_set_option: min-sum has no correlated form; set QEC_OPT_CORRELATED to 0 first");
        if (value && d->bp_schedule)
            return fail(QEC_ERR_UNSUPPORTED,
                        "qec_decoder_set_option: min-sum is built for the flooding schedule; set QEC_OPT_BP_SCHEDULE to 0 "
                        "(flooding) first");
        if (!value && d->has_syn)
            return fail(QEC_ERR_UNSUPPORTED,
                        "qec_decoder_set_option: syndrome priors are built for min-sum; clear them "
                        "(qec_decoder_set_syndrome_priors(dec, NULL, NULL)) before QEC_OPT_BP_METHOD = 0");
        d->bp_method = value;
        return QEC_OK;
    case QEC_OPT_MINSUM_SCALE:
        if (value < 1 || value > 256)
            return fail(QEC_ERR_ARG, "qec_decoder_set_option: QEC_OPT_MINSUM_SCALE is 1 .. 256 (alpha = value / 256)");
        d->minsum_scale = value;
        return QEC_OK;
    case QEC_OPT_MINSUM_SCHEDULE:
        if (value != 0 && value != 1)
            return fail(QEC_ERR_ARG, "qec_decoder_set_option: QEC_OPT_MINSUM_SCHEDULE is 0 (flooding) or 1 (layered)");
        if (value && d->parts.empty() && !d->cpu && d->engine != QEC_ENGINE_SPARSE)
            return fail(QEC_ERR_UNSUPPORTED,
                        "qec_decoder_set_option: QEC_OPT_MINSUM_SCHEDULE = 1 (layered) is a schedule of min-sum, which the "
                        "wave-circulant engine does not run; create the decoder with QEC_ENGINE_SPARSE (engine \"sparse\")");
        d->minsum_schedule = value;
        return QEC_OK;
    case QEC_OPT_MINSUM_WAVE:
        return set_wave_option(d, value, d->minsum_wave, "QEC_OPT_MINSUM_WAVE", "min-sum", "decodes by min-sum",
                               select_wave_minsum);
    case QEC_OPT_RELAY_WAVE:
        return set_wave_option(d, value, d->relay_wave, "QEC_OPT_RELAY_WAVE", "relay", "runs the relay",
                               select_wave_relay);
    case QEC_OPT_OSD_CS_SECTORS:
        return fail(QEC_ERR_ARG, "qec_decoder_set_option: QEC_OPT_OSD_CS_SECTORS is read only");
    case QEC_OPT_LAST_PATH: return fail(QEC_ERR_ARG, "qec_decoder_set_option: QEC_OPT_LAST_PATH is read only");
    default: return fail(QEC_ERR_ARG, "qec_decoder_set_option: unknown option");
    }
}

// qec_decoder_set_priors and qec_decoder_set_pauli_channel: validates and installs the marginal priors (host copy,
// device buffer, OSD weight tables, every part of a group) together with the correlated form's conditional tables --
// cond4 = c0_X, c1_X, c0_Z, c1_Z [n each], or nullptr for plain priors (c0 = c1 = the marginal) -- and the channel
// (pauli3 = pX, pY, pZ [n each], or nullptr: no channel from here on).  `who` names the public call in the texts.
static int install_priors(qec_decoder* d, const char* who, const float* priorX, const float* priorZ, const float* cond4,
                          const float* pauli3)
{
    if (!d->cpu && d->engine != QEC_ENGINE_SPARSE)
        return fail(QEC_ERR_UNSUPPORTED,
                    std::string(who) + ": the wave-circulant engine decodes with one error probability (its hard-message "
                    "shortcuts are proven for one p'); create the decoder with QEC_ENGINE_SPARSE (engine \"sparse\")");
    const int n = d->code->n;
    for (int sec = 0; sec < 2; ++sec) {
        const float* pr = sec ? priorZ : priorX;
        for (int v = 0; v < n; ++v)
            if (!(pr[v] >= 0.0f && pr[v] <= 1.0f))  // a NaN fails both comparisons
                return fail(QEC_ERR_ARG, std::string(who) + ": prior" + (sec ? "Z[" : "X[") + std::to_string(v) +
                                             "] = " + std::to_string(pr[v]) + " is not in [0, 1]");
    }
    if (d->odev && d->osd_score == 1 && d->osd_order > 0) {  // the weighted sweep would run from here on
        const std::string why = osd_dev_unsupported(*d->oplan, d->osd_order, true);
        if (!why.empty()) return fail(QEC_ERR_UNSUPPORTED, why);
    }
    std::vector<float> host(2 * (size_t)n);
    std::memcpy(host.data(), priorX, n * sizeof(float));
    std::memcpy(host.data() + n, priorZ, n * sizeof(float));
    std::vector<int32_t> wts(host.size());  // the sweep's weight tables (QEC_OPT_OSD_SCORE = 1)
    for (size_t i = 0; i < host.size(); ++i) wts[i] = osd_weight(host[i]);
    std::vector<float> llr(host.size());    // the channel LLRs of the min-sum form (QEC_OPT_BP_METHOD = 1)
    for (size_t i = 0; i < host.size(); ++i) llr[i] = minsum_llr(host[i]);
    std::vector<float> cond(4 * (size_t)n), pauli;
    if (cond4) {
        std::memcpy(cond.data(), cond4, cond.size() * sizeof(float));
    } else {  // independent marginals carry no correlation: both conditionals are the marginal
        for (int sec = 0; sec < 2; ++sec)
            for (int k = 0; k < 2; ++k) std::memcpy(cond.data() + (size_t)(2 * sec + k) * n, sec ? priorZ : priorX, n * sizeof(float));
    }
    std::vector<uint64_t> thr;
    if (pauli3) {
        pauli.assign(pauli3, pauli3 + 3 * (size_t)n);
        thr.resize(3 * (size_t)n);
        for (int v = 0; v < n; ++v) {
            const double x = pauli3[v], y = pauli3[n + v], z = pauli3[2 * n + v];
            thr[v] = (uint64_t)(x * 4294967296.0);
            thr[n + v] = (uint64_t)((x + y) * 4294967296.0);
            thr[2 * n + v] = (uint64_t)(std::min(1.0, (x + y) + z) * 4294967296.0);
        }
    }
    for (qec_decoder* p : d->parts) {
        const int rc = install_priors(p, who, priorX, priorZ, cond4, pauli3);
        if (rc) return rc;
    }
    if (d->parts.empty() && !d->cpu) {
        QEC_DEVICE_SCOPE(d->device);
        // synchronous: the handle's last launch may still read the buffers this call rewrites
        QEC_HIP_CHECK(hipStreamSynchronize(d->stream));
        if (d->ws_used) QEC_HIP_CHECK(hipEventSynchronize(d->ws_ev));
        try {
            d->dpri.reserve(host.size());
            d->dosw.reserve(wts.size());
            d->dcond.reserve(cond.size());
            d->dmllr.reserve(llr.size());
            if (pauli3) d->dpth.reserve(thr.size());
        } catch (const std::exception& ex) {
            return fail(QEC_ERR_NOMEM, std::string(who) + ": " + ex.what());
        }
        QEC_HIP_CHECK(hipMemcpy(d->dpri.data(), host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
        QEC_HIP_CHECK(hipMemcpy(d->dosw.data(), wts.data(), wts.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        QEC_HIP_CHECK(hipMemcpy(d->dcond.data(), cond.data(), cond.size() * sizeof(float), hipMemcpyHostToDevice));
        QEC_HIP_CHECK(hipMemcpy(d->dmllr.data(), llr.data(), llr.size() * sizeof(float), hipMemcpyHostToDevice));
        if (pauli3) QEC_HIP_CHECK(hipMemcpy(d->dpth.data(), thr.data(), thr.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    }
    d->priors.swap(host);
    d->osw.swap(wts);
    d->cond.swap(cond);
    d->mllr.swap(llr);
    d->pauli.swap(pauli);
    d->has_channel = pauli3 != nullptr;
    d->has_priors = true;
    return QEC_OK;
}

static void clear_priors(qec_decoder* d)
{
    // the handle behaves as one that never had priors or a channel (the device buffers are kept)
    for (qec_decoder* p : d->parts) p->has_priors = p->has_channel = false;
    d->has_priors = d->has_channel = false;
}

int qec_decoder_set_priors(qec_decoder* d, const float* priorX, const float* priorZ)
{
    if (!d) return fail(QEC_ERR_ARG, "qec_decoder_set_priors: null decoder");
    if ((priorX == nullptr) != (priorZ == nullptr))
        return fail(QEC_ERR_ARG, "qec_decoder_set_priors: priorX and priorZ must both be given, or both be NULL (clear)");
    if (!priorX) {
        clear_priors(d);
        return QEC_OK;
    }
    return install_priors(d, "qec_decoder_set_priors", priorX, priorZ, nullptr, nullptr);
}

int qec_decoder_set_pauli_channel(qec_decoder* d, const float* pX, const float* pY, const float* pZ)
{
    if (!d) return fail(QEC_ERR_ARG, "qec_decoder_set_pauli_channel: null decoder");
    const int nulls = (pX == nullptr) + (pY == nullptr) + (pZ == nullptr);
    if (nulls == 3) {
        clear_priors(d);
        return QEC_OK;
    }
    if (nulls) return fail(QEC_ERR_ARG, "qec_decoder_set_pauli_channel: pX, pY and pZ must all be given, or all be NULL (clear)");
    if (!d->cpu && d->engine != QEC_ENGINE_SPARSE)
        return fail(QEC_ERR_UNSUPPORTED,
                    "qec_decoder_set_pauli_channel: the wave-circulant engine decodes with one error probability (its "
                    "hard-message shortcuts are proven for one p'); create the decoder with QEC_ENGINE_SPARSE (engine \"sparse\")");
    const int n = d->code->n;
    const float* arr[3] = {pX, pY, pZ};
    for (int a = 0; a < 3; ++a)
        for (int v = 0; v < n; ++v)
            if (!(arr[a][v] >= 0.0f && arr[a][v] <= 1.0f))  // a NaN fails both comparisons
                return fail(QEC_ERR_ARG, std::string("qec_decoder_set_pauli_channel: p") + "XYZ"[a] + "[" + std::to_string(v) +
                                             "] = " + std::to_string(arr[a][v]) + " is not in [0, 1]");
    std::vector<float> mar(2 * (size_t)n), cond(4 * (size_t)n), pauli(3 * (size_t)n);
    auto ratio = [](double num, double den) { return den == 0.0 ? 0.5f : (float)std::min(1.0, num / den); };
    for (int v = 0; v < n; ++v) {
        const double x = pX[v], y = pY[v], z = pZ[v];
        if (!((x + y) + z <= 1.0))
            return fail(QEC_ERR_ARG, "qec_decoder_set_pauli_channel: pX[" + std::to_string(v) + "] + pY[" + std::to_string(v) +
                                         "] + pZ[" + std::to_string(v) + "] = " + std::to_string((x + y) + z) + " is above 1");
        mar[v] = (float)(x + y);
        mar[n + v] = (float)(z + y);
        cond[v] = ratio(x, 1.0 - (z + y));          // cX0
        cond[n + v] = ratio(y, z + y);              // cX1
        cond[2 * n + v] = ratio(z, 1.0 - (x + y));  // cZ0
        cond[3 * n + v] = ratio(y, x + y);          // cZ1
        pauli[v] = pX[v]; pauli[n + v] = pY[v]; pauli[2 * n + v] = pZ[v];
    }
    return install_priors(d, "qec_decoder_set_pauli_channel", mar.data(), mar.data() + n, cond.data(), pauli.data());
}

int qec_decoder_get_pauli_channel(const qec_decoder* d, float* pX, float* pY, float* pZ)
{
    if (!d) return fail(QEC_ERR_ARG, "qec_decoder_get_pauli_channel: null decoder");
    if (!d->has_channel) return 0;
    const int n = d->code->n;
    float* out[3] = {pX, pY, pZ};
    for (int a = 0; a < 3; ++a)
        if (out[a]) std::memcpy(out[a], d->pauli.data() + (size_t)a * n, n * sizeof(float));
    return 1;
}

int qec_decoder_get_conditional_priors(const qec_decoder* d, float* cZ0, float* cZ1, float* cX0, float* cX1)
{
    if (!d) return fail(QEC_ERR_ARG, "qec_decoder_get_conditional_priors: null decoder");
    if (!d->has_channel) return 0;
    const int n = d->code->n;
    float* out[4] = {cX0, cX1, cZ0, cZ1};  // the tables' order in the handle
    for (int a = 0; a < 4; ++a)
        if (out[a]) std::memcpy(out[a], d->cond.data() + (size_t)a * n, n * sizeof(float));
    return 1;
}

int qec_correlated_priors(float p, float* c0, float* c1)
{
    if (!c0 || !c1) return fail(QEC_ERR_ARG, "qec_correlated_priors: bad argument");
    correlated_priors(p, c0, c1);
    return QEC_OK;
}

int qec_decoder_get_priors(const qec_decoder* d, float* priorX, float* priorZ)
{
    if (!d) return fail(QEC_ERR_ARG, "qec_decoder_get_priors: null decoder");
    if (!d->has_priors) return 0;
    const int n = d->code->n;
    if (priorX) std::memcpy(priorX, d->priors.data(), n * sizeof(float));
    if (priorZ) std::memcpy(priorZ, d->priors.data() + n, n * sizeof(float));
    return 1;
}

int qec_minsum_llr(float prior, float* llr)
{
    if (!llr) return fail(QEC_ERR_ARG, "qec_minsum_llr: bad argument");
    *llr = minsum_llr(prior);
    return QEC_OK;
}

int qec_decoder_get_minsum_llr(const qec_decoder* d, float* llrX, float* llrZ)
{
    if (!d) return fail(QEC_ERR_ARG, "qec_decoder_get_minsum_llr: null decoder");
    if (!d->has_priors)
        return fail(QEC_ERR_ARG, "qec_decoder_get_minsum_llr: the decoder has no priors (qec_decoder_set_priors)");
    const int n = d->code->n;
    if (llrX) std::memcpy(llrX, d->mllr.data(), n * sizeof(float));
    if (llrZ) std::memcpy(llrZ, d->mllr.data() + n, n * sizeof(float));
    return QEC_OK;
}

// Installs validated relay tables ([legs][sector][n]) on a handle and on every part of a group
static int install_relay(qec_decoder* d, const std::vector<float>& tab, int legs, int solutions)
{
    for (qec_decoder* p : d->parts) {
        const int rc = install_relay(p, tab, legs, solutions);
        if (rc) return rc;
    }
    if (d->parts.empty() && !d->cpu) {
        QEC_DEVICE_SCOPE(d->device);
        // synchronous: the handle's last launch may still read the buffer this call rewrites
        QEC_HIP_CHECK(hipStreamSynchronize(d->stream));
        if (d->ws_used) QEC_HIP_CHECK(hipEventSynchronize(d->ws_ev));
        try {
            d->drelay.reserve(2 * (size_t)kRelayMaxEntries);  // once, at the largest legal size: it never moves
        } catch (const std::exception& ex) {
            return fail(QEC_ERR_NOMEM, std::string("qec_decoder_set_relay: ") + ex.what());
        }
        const int rc = sparse_plan_relay_reserve(d->sparse);
        if (rc) return rc;
        QEC_HIP_CHECK(hipMemcpy(d->drelay.data(), tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    d->relay = tab;
    d->relay_legs = legs;
    d->relay_solutions = solutions;
    return QEC_OK;
}

int qec_decoder_set_relay(qec_decoder* d, const float* gammaX, const float* gammaZ, int legs, int solutions)
{
    if (!d) return fail(QEC_ERR_ARG, "qec_decoder_set_relay: null decoder");
    if (!gammaX && !gammaZ && legs == 0 && solutions == 0) {  // clear: the handle behaves as one that never had tables
        for (qec_decoder* p : d->parts) p->relay_legs = p->relay_solutions = 0;
        d->relay_legs = d->relay_solutions = 0;
        return QEC_OK;
    }
    if (!gammaX || !gammaZ)
        return fail(QEC_ERR_ARG, "qec_decoder_set_relay: gammaX and gammaZ must both be given, or (NULL, NULL, 0, 0) to clear");
    const int n = d->code->n;
    if (legs < 1 || legs > kRelayMaxLegs || (long long)legs * n > kRelayMaxEntries)
        return fail(QEC_ERR_ARG, "qec_decoder_set_relay: legs is 1 .. 1024 with legs * n <= 2^22");
    if (solutions < 1 || solutions > kRelayMaxSolutions)
        return fail(QEC_ERR_ARG, "qec_decoder_set_relay: solutions is 1 .. 64");
    for (int sec = 0; sec < 2; ++sec) {
        const float* g = sec ? gammaZ : gammaX;
        for (size_t i = 0; i < (size_t)legs * n; ++i)
            if (!(g[i] >= -1.0f && g[i] <= 1.0f))  // a NaN fails both comparisons
                return fail(QEC_ERR_ARG, std::string("qec_decoder_set_relay: gamma") + (sec ? "Z[" : "X[") + std::to_string(i / n) +
                                             "][" + std::to_string(i % n) + "] = " + std::to_string(g[i]) + " is not in [-1, 1]");
    }
    if (d->has_syn)
        return fail(QEC_ERR_UNSUPPORTED,
                    "qec_decoder_set_relay: the relay's legs have no form under syndrome priors; clear them "
                    "(qec_decoder_set_syndrome_priors(dec, NULL, NULL)) first");
    bool sparse = true;
    for (const qec_decoder* p : parts_of(d)) sparse = sparse && (p->cpu || p->engine == QEC_ENGINE_SPARSE);
    if (!sparse)
        return fail(QEC_ERR_UNSUPPORTED,
                    "qec_decoder_set_relay: the relay is min-sum with memory, which is not built for the wave-circulant engine; "
                    "create the decoder with QEC_ENGINE_SPARSE (engine \"sparse\")");
    std::vector<float> tab(2 * (size_t)legs * n);
    for (int l = 0; l < legs; ++l) {
        std::memcpy(tab.data() + (2 * (size_t)l) * n, gammaX + (size_t)l * n, n * sizeof(float));
        std::memcpy(tab.data() + (2 * (size_t)l + 1) * n, gammaZ + (size_t)l * n, n * sizeof(float));
    }
    return install_relay(d, tab, legs, solutions);
}

int qec_decoder_get_relay(const qec_decoder* d, float* gammaX, float* gammaZ, int* legs, int* solutions)
{
    if (!d) return fail(QEC_ERR_ARG, "qec_decoder_get_relay: null decoder");
    if (legs) *legs = d->relay_legs;
    if (solutions) *solutions = d->relay_solutions;
    const int n = d->code->n;
    for (int l = 0; l < d->relay_legs; ++l) {
        if (gammaX) std::memcpy(gammaX + (size_t)l * n, d->relay.data() + (2 * (size_t)l) * n, n * sizeof(float));
        if (gammaZ) std::memcpy(gammaZ + (size_t)l * n, d->relay.data() + (2 * (size_t)l + 1) * n, n * sizeof(float));
    }
    return QEC_OK;
}

// Installs validated syndrome priors (q and their LLRs, sector X [mX] then Z [mZ]) on a handle and on every part of a group
static int install_syndrome_priors(qec_decoder* d, const std::vector<float>& q, const std::vector<float>& mu)
{
    for (qec_decoder* p : d->parts) {
        const int rc = install_syndrome_priors(p, q, mu);
        if (rc) return rc;
    }
    if (d->parts.empty() && !d->cpu) {
        QEC_DEVICE_SCOPE(d->device);
        // synchronous: the handle's last launch may still read the buffer this call rewrites
        QEC_HIP_CHECK(hipStreamSynchronize(d->stream));
        if (d->ws_used) QEC_HIP_CHECK(hipEventSynchronize(d->ws_ev));
        try {
            d->dsyn.reserve(2 * q.size());
        } catch (const std::exception& ex) {
            return fail(QEC_ERR_NOMEM, std::string("qec_decoder_set_syndrome_priors: ") + ex.what());
        }
        QEC_HIP_CHECK(hipMemcpy(d->dsyn.data(), mu.data(), mu.size() * sizeof(float), hipMemcpyHostToDevice));
        QEC_HIP_CHECK(hipMemcpy(d->dsyn.data() + mu.size(), q.data(), q.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    d->synq = q;
    d->synmu = mu;
    d->has_syn = true;
    return QEC_OK;
}

int qec_decoder_set_syndrome_priors(qec_decoder* d, const float* qX, const float* qZ)
{
    const std::string who = "qec_decoder_set_syndrome_priors: ";
    if (!d) return fail(QEC_ERR_ARG, who + "null decoder");
    if (!qX && !qZ) {  // clear: the handle behaves as one that never had them (the device buffer is kept)
        for (qec_decoder* p : d->parts) p->has_syn = false;
        d->has_syn = false;
        return QEC_OK;
    }
    if (!qX || !qZ) return fail(QEC_ERR_ARG, who + "qX and qZ must both be given, or both be NULL (clear)");
    const int mX = d->code->mX, mZ = d->code->mZ;
    for (int sec = 0; sec < 2; ++sec) {
        const float* q = sec ? qZ : qX;
        for (int c = 0; c < (sec ? mZ : mX); ++c)
            if (!(q[c] >= 0.0f && q[c] <= 1.0f))  // a NaN fails both comparisons
                return fail(QEC_ERR_ARG, who + "q" + (sec ? "Z[" : "X[") + std::to_string(c) + "] = " + std::to_string(q[c]) +
                                             " is not in [0, 1]");
    }
    bool sparse = true;
    for (const qec_decoder* p : parts_of(d)) sparse = sparse && (p->cpu || p->engine == QEC_ENGINE_SPARSE);
    if (!sparse)
        return fail(QEC_ERR_UNSUPPORTED, who + "syndrome priors are a form of min-sum, which is not built for the wave-circulant "
                                               "engine; create the decoder with QEC_ENGINE_SPARSE (engine \"sparse\")");
    if (d->bp_method != 1)
        return fail(QEC_ERR_UNSUPPORTED, who + "syndrome priors are built for min-sum; set QEC_OPT_BP_METHOD to 1 first");
    if (d->relay_legs > 0)
        return fail(QEC_ERR_UNSUPPORTED, who + "the relay's legs have no form under syndrome priors; clear the relay tables "
                                               "(qec_decoder_set_relay(dec, NULL, NULL, 0, 0)) first");
    if (d->osd)
        return fail(QEC_ERR_UNSUPPORTED, who + "the OSD stage solves H e = s exactly, which is not the problem under syndrome "
                                               "priors; set QEC_OPT_OSD to 0 first");
    std::vector<float> q((size_t)mX + mZ), mu(q.size());
    std::memcpy(q.data(), qX, mX * sizeof(float));
    std::memcpy(q.data() + mX, qZ, mZ * sizeof(float));
    for (size_t i = 0; i < q.size(); ++i) mu[i] = minsum_llr(q[i]);
    return install_syndrome_priors(d, q, mu);
}

int qec_decoder_get_syndrome_priors(const qec_decoder* d, float* qX, float* qZ)
{
    if (!d) return fail(QEC_ERR_ARG, "qec_decoder_get_syndrome_priors: null decoder");
    if (!d->has_syn) return 0;
    const int mX = d->code->mX, mZ = d->code->mZ;
    if (qX) std::memcpy(qX, d->synq.data(), mX * sizeof(float));
    if (qZ) std::memcpy(qZ, d->synq.data() + mX, mZ * sizeof(float));
    return 1;
}

int qec_decoder_get_osd_weights(const qec_decoder* d, int32_t* wX, int32_t* wZ)
{
    if (!d) return fail(QEC_ERR_ARG, "qec_decoder_get_osd_weights: null decoder");
    if (!d->has_priors) return 0;
    const int n = d->code->n;
    if (wX) std::memcpy(wX, d->osw.data(), n * sizeof(int32_t));
    if (wZ) std::memcpy(wZ, d->osw.data() + n, n * sizeof(int32_t));
    return 1;
}

int qec_decoder_get_option(const qec_decoder* d, int option, int* value)
{
    if (!d || !value) return fail(QEC_ERR_ARG, "qec_decoder_get_option: bad argument");
    switch (option) {
    case QEC_OPT_HARD_PATHS: *value = d->hard_paths; return QEC_OK;
    case QEC_OPT_CYCLE_JUMP: *value = d->cycle_jump; return QEC_OK;
    case QEC_OPT_NEAR_HARD_JUMP: *value = d->near_hard; return QEC_OK;
    case QEC_OPT_NEAR_PROBE: *value = d->near_probe; return QEC_OK;
    case QEC_OPT_LIGHT_MEMO: *value = d->light_memo; return QEC_OK;
    case QEC_OPT_SCHEDULE: *value = d->schedule; return QEC_OK;
    case QEC_OPT_SECTOR_SPLIT: *value = d->sector_split; return QEC_OK;
    case QEC_OPT_PHASE_STATS: *value = d->phase_stats; return QEC_OK;
    case QEC_OPT_TRIAGE: *value = d->triage; return QEC_OK;
    case QEC_OPT_LAST_PATH: *value = d->parts.empty() ? d->last_path : d->parts[0]->last_path; return QEC_OK;
    case QEC_OPT_MC_DECODE_TIME: *value = d->mc_time; return QEC_OK;
    case QEC_OPT_OSD: *value = d->osd; return QEC_OK;
    case QEC_OPT_OSD_ITERATIONS: *value = d->osd_iters; return QEC_OK;
    case QEC_OPT_OSD_SWEEP: *value = d->osd_sweep; return QEC_OK;
    case QEC_OPT_OSD_SECTORS: {
        unsigned long long t = d->osd_sectors;
        for (const qec_decoder* p : d->parts) t += p->osd_sectors;
        *value = (int)std::min<unsigned long long>(t, 0x7FFFFFFFull);
        return QEC_OK;
    }
    case QEC_OPT_OSD_ORDER: *value = d->osd_order; return QEC_OK;
    case QEC_OPT_OSD_SCORE: *value = d->osd_score; return QEC_OK;
    case QEC_OPT_CORRELATED: *value = d->correlated; return QEC_OK;
    case QEC_OPT_BP_SCHEDULE: *value = d->bp_schedule; return QEC_OK;
    case QEC_OPT_BP_METHOD: *value = d->bp_method; return QEC_OK;
    case QEC_OPT_MINSUM_SCALE: *value = d->minsum_scale; return QEC_OK;
    case QEC_OPT_MINSUM_WAVE: *value = d->minsum_wave; return QEC_OK;
    case QEC_OPT_MINSUM_SCHEDULE: *value = d->minsum_schedule; return QEC_OK;
    case QEC_OPT_RELAY_WAVE: *value = d->relay_wave; return QEC_OK;
    case QEC_OPT_OSD_CS_SECTORS: {
        unsigned long long t = d->osd_cs_sectors;
        for (const qec_decoder* p : d->parts) t += p->osd_cs_sectors;
        *value = (int)std::min<unsigned long long>(t, 0x7FFFFFFFull);
        return QEC_OK;
    }
    default: return fail(QEC_ERR_ARG, "qec_decoder_get_option: unknown option");
    }
}

}  // extern "C"

namespace {

// QEC_OPT_SCHEDULE = 1 orders batches from this size on (below it the extra launches cost more
// than the tail they remove) and, with one syndrome per wave (P > 32), up to kScheduleMaxSingle:
// there the order pass reads every syndrome once more (P61: 177 us per 2^20) while the tail it
// removes stays about one long sector (~0.1 ms); P61 at 2^20: 118.7 M/s unordered vs 116.9 M/s,
// at 131 072: 101 M/s vs 113 M/s (profiles/r02/ab_schedule.txt).  Several syndromes per wave (P7)
// always gain: similar syndromes then share waves (1.56 G/s vs 0.88 G/s at 2^20).
// Under the syndrome stop at low p nearly every sector stops at iteration 0 or 1, so there is no
// tail to remove and the pass is pure cost: below kScheduleSyndromeMinP it stays off there
// (P61, 65 536 per batch: p = 0.001 290 vs 266 M/s, 0.002 263 vs 257 off vs on, but 0.005 190 vs
// 197, 0.01 124 vs 143; 262 144 at p = 0.002: 0.450 vs 0.521 ms; profiles/r02/psweep_sched{0,1}_r02s3g.json,
// profiles/r02/cmp_options_r02s3zb.txt).  With sector launches or split waves each sector's waves
// can follow that sector's own weight (schedule_sector_order), which pays for P61 at 2^20 too: the
// bit-row headline 143.1 vs 140.6 M/s ordered vs not (profiles/r04/bench/configs3_*).
constexpr long long kScheduleMinBatch = 4096;
constexpr long long kScheduleMaxSingle = 1LL << 19;
constexpr float kScheduleSyndromeMinP = 0.004f;
constexpr float kTriageMaxP = 0.01f;  // QEC_OPT_TRIAGE = 1 triages syndrome-stop batches up to this p
// QEC_OPT_SECTOR_SPLIT = 1 splits batches above this size only when they get the per-sector order
constexpr long long kSplitOrderedMinBatch = 1LL << 19;

int hard_path_bits(const qec_decoder* d)
{
    return (d->hard_paths ? (QEC_HP_FORMS | (d->cycle_jump ? QEC_HP_CYCLE : 0) | (d->near_hard ? QEC_HP_NEAR | (d->near_probe ? QEC_HP_NEAR_PROBE : 0) : 0)) : 0) |
           (d->phase_stats ? QEC_HP_PHASE : 0);
}

// QEC_OPT_TRIAGE: 1 (auto) and 3 (auto, never the fused Monte-Carlo kernel) up to kTriageMaxP, 2 always
bool triage_on(const qec_decoder* d, float p)
{
    return !d->phase_stats && (d->triage == 2 || ((d->triage == 1 || d->triage == 3) && p <= kTriageMaxP));
}

// One decode launch of a single-device handle on device buffers.  Outputs: byte form (eX, eZ,
// flags) or, with rec non-null, the packed decision records.
// sbits: sX / sZ are bit rows ([B][ceil(m/32)] words, the Monte-Carlo pipeline's layout; wave-circulant
// engine only), else byte rows
// rec_stride: record row stride (0: 2 nb + 1, the public layout; the Monte-Carlo pipeline pads rows to
// whole words for its statistics kernel; wave-circulant engine only)
int dispatch_decode(qec_decoder* d, const uint8_t* sX, const uint8_t* sZ, long long B, float p, int maxIter, int stop,
                    uint8_t* eX, uint8_t* eZ, uint8_t* flags, uint8_t* rec, int32_t* iters, float* q, hipStream_t st,
                    bool sbits = false, int rec_stride = 0, uint8_t* fX = nullptr, uint8_t* fZ = nullptr)
{
    if (B <= 0) return QEC_OK;
    const Code& c = *d->code;
    int rc = ws_acquire(d, st);
    if (rc) return rc;
    if (!d->soft_on()) {  // qec_decode_batch_soft on a handle without syndrome priors: no measurement bit is flipped
        if (fX) QEC_HIP_CHECK(hipMemsetAsync(fX, 0, (size_t)B * c.mX, st));
        if (fZ) QEC_HIP_CHECK(hipMemsetAsync(fZ, 0, (size_t)B * c.mZ, st));
    }
    d->last_path = (sbits ? QEC_PATH_BIT_ROWS : 0) | (rec != nullptr ? QEC_PATH_RECORDS : 0);
    if (d->engine == QEC_ENGINE_SPARSE) {
        d->last_path |= QEC_PATH_SPARSE;
        if (sbits) return fail(QEC_ERR_UNSUPPORTED, "decode: bit-row syndromes need the wave-circulant engine");
        if (rec_stride > 0 && rec_stride != 2 * ((c.n + 7) / 8) + 1)
            return fail(QEC_ERR_UNSUPPORTED, "decode: padded record rows need the wave-circulant engine");
        if (rec != nullptr) {  // byte outputs into the handle's staging, then packed
            if ((rc = ws_reserve(d->eX, (size_t)B * c.n, st, "decode")) || (rc = ws_reserve(d->eZ, (size_t)B * c.n, st, "decode")) ||
                (rc = ws_reserve(d->flags, (size_t)B, st, "decode")))
                return rc;
            eX = d->eX.data(); eZ = d->eZ.data(); flags = d->flags.data();
        }
        SparseDecode sd;
        sd.sX = sX; sd.sZ = sZ; sd.B = B; sd.errorProbability = p; sd.maxIter = maxIter; sd.stop = stop;
        sd.eX = eX; sd.eZ = eZ; sd.flags = flags; sd.iters = iters; sd.q = q;
        sd.prior = d->prior_dev();
        // QEC_OPT_CORRELATED, read at the call: the CORR kernels, with the handle's conditional tables or the scalar pair
        sd.corr = d->correlated;
        sd.cond = d->cond_dev();
        if (sd.corr) {
            correlated_priors(p, &sd.c0, &sd.c1);
            d->last_path |= QEC_PATH_CORRELATED;
        }
        // QEC_OPT_BP_SCHEDULE, read at the call too: the SERIAL kernels (never together with corr: set_option refuses)
        sd.serial = d->bp_schedule;
        if (sd.serial) d->last_path |= QEC_PATH_SERIAL;
        // QEC_OPT_BP_METHOD and QEC_OPT_MINSUM_SCALE, read at the call: the MINSUM kernels under the channel LLR of p',
        // formed here on the host, or under the handle's LLR tables (never with corr or serial: set_option refuses)
        sd.minsum = d->minsum();
        if (sd.minsum) {
            sd.lam = minsum_llr(2.0f / 3.0f * p);
            sd.llr = d->llr_dev();
            d->last_path |= QEC_PATH_MINSUM;
            // qec_decoder_set_relay, read at the call: the RELAY kernels under the handle's tables
            sd.gamma = d->relay_dev();
            if (sd.gamma) {
                sd.legs = d->relay_legs;
                sd.solutions = d->relay_solutions;
                sd.relay_weight = d->relay_w_dev();
                d->last_path |= QEC_PATH_RELAY;
            }
            // QEC_OPT_MINSUM_SCHEDULE, read at the call: the LAYERED kernels (plain min-sum only: the relay's legs flood)
            sd.layered = d->layered_on();
            if (sd.layered) d->last_path |= QEC_PATH_SERIAL;
            // qec_decoder_set_syndrome_priors, read at the call: the SOFT kernels under the handle's table
            sd.mu = d->mu_dev();
            if (sd.mu) {
                sd.fX = fX;
                sd.fZ = fZ;
                d->last_path |= QEC_PATH_SOFT;
            }
        }
        // QEC_OPT_MINSUM_WAVE, read at the call: plain min-sum in the wave layout (set_option has checked the code)
        if (sd.minsum && sd.gamma == nullptr && d->minsum_wave) {
            d->last_path |= QEC_PATH_WAVE;
            rc = launch_wave_minsum(select_wave_minsum(c), c, sd, st);
        } else if (sd.minsum && sd.gamma != nullptr && d->relay_wave) {
            // QEC_OPT_RELAY_WAVE, read at the call: the relay in the wave layout (set_option has checked the code)
            d->last_path |= QEC_PATH_WAVE;
            rc = launch_wave_relay(select_wave_relay(c), c, sd, st);
        } else {
            rc = launch_decode_sparse(d->sparse, sd, st);
        }
        if (!rc && rec != nullptr) rc = launch_pack_decisions(eX, eZ, flags, B, c.n, rec, st);
        if (rc) return rc;
        return ws_release(d, st);
    }
    const int hp = hard_path_bits(d);
    // syndrome stop on bit rows into records (the Monte-Carlo pipeline): triage iteration 0 for 64
    // syndromes per wave, then decode only the sectors it passes on (triage.hip, list mode)
    // Above p = 0.01 most sectors go on past iteration 0 (P61 at p = 0.02: 2.2 iterations per sector)
    // and the list-mode decode of nearly the whole batch loses to the ordered one-wave-per-syndrome
    // launch (140 vs 178 M syn/s at p = 0.02, 6.4 vs 8.3 at 0.1; 1.47 G vs 0.50 G at 0.002,
    // profiles/r03/psweep_triage.json), so the triage stays off there.
    uint32_t pats[4];
    if (triage_on(d, p) && stop == QEC_STOP_SYNDROME && sbits && rec != nullptr && q == nullptr &&
        maxIter >= 2 && B < (1LL << 31) && decode_has_list(d->variant) && triage_supported(c) && triage_aligned(sX, sZ) &&
        (reinterpret_cast<uintptr_t>(iters) & 7u) == 0 &&  // the triage stores both counts as one 8-byte word
        decode_pattern_masks(d->variant, p, pats)) {
        if ((rc = ws_reserve(d->merge, (size_t)B, st, "decode")) || (rc = ws_reserve(d->tlist, 2 * (size_t)B + 2, st, "decode")))
            return rc;
        int32_t* lX = d->tlist.data();
        int32_t* lZ = lX + B;
        uint32_t* cnt = reinterpret_cast<uint32_t*>(lZ + B);
        QEC_HIP_CHECK(hipMemsetAsync(cnt, 0, 2 * sizeof(uint32_t), st));
        rc = launch_triage(c, reinterpret_cast<const uint32_t*>(sX), reinterpret_cast<const uint32_t*>(sZ), B, pats, rec,
                           iters, d->merge.data(), lX, lZ, cnt, st, rec_stride);
        if (!rc)
            rc = launch_decode_list(d->variant, c, sX, sZ, B, p, maxIter, hp, rec, iters, d->merge.data(), lX, lZ, cnt, st,
                                    rec_stride, false, 1, ws_done(d, st));
        if (rc) return rc;
        d->last_path |= QEC_PATH_TRIAGE;
        return ws_release(d, st, true);
    }
    // QEC_OPT_SECTOR_SPLIT = 1 resolved per launch (the variant's measured choice for this stop, batch and p)
    int split_opt = decode_sector_mode(d->variant, stop, d->sector_split, B, p);
    const bool split_auto = d->sector_split == 1;
    bool split = !d->phase_stats && decode_uses_split(d->variant, stop, split_opt, B);
    bool need_merge = !d->phase_stats && decode_needs_merge(d->variant, stop, split_opt, B);
    const bool single = 2 * c.P > 64;  // one syndrome per wave
    bool sectors = split || need_merge;  // split waves or sector launches
    const bool auto_on = B >= kScheduleMinBatch &&
                         (!single || B <= kScheduleMaxSingle || (sectors && schedule_sector_order(B, sbits, c.mX, c.mZ))) &&
                         !(stop == QEC_STOP_SYNDROME && p < kScheduleSyndromeMinP);
    const bool ordered = B > 1 && B <= schedule_max_batch() && (d->schedule >= 2 || (d->schedule == 1 && auto_on));
    const int method = d->schedule == 3 ? QEC_ORDER_LOCAL : d->schedule == 4 ? QEC_ORDER_ONE_LAUNCH : QEC_ORDER_GLOBAL;
    // The tuned split above kSplitOrderedMinBatch was measured only with the per-sector order (round 2:
    // in total-weight order one wave per group won from 2^19 on); without that order keep one wave per group
    if (split && split_auto && B > kSplitOrderedMinBatch &&
        !(ordered && method == QEC_ORDER_GLOBAL && schedule_sector_order(B, sbits, c.mX, c.mZ))) {
        split_opt = 0;
        split = false;
        need_merge = !d->phase_stats && decode_needs_merge(d->variant, stop, split_opt, B);
        sectors = need_merge;
    }
    if (need_merge && (rc = ws_reserve(d->merge, (size_t)B, st, "decode"))) return rc;
    const int32_t* perm = nullptr;
    bool zeroed = false, perm_sectors = false;
    if (ordered) {
        if ((rc = ws_reserve(d->sched, schedule_workspace_bytes(B, c.mX, c.mZ), st, "decode: dispatch order")))
            return rc;
        int32_t* pm = nullptr;
        // a sector-split launch merges its flags in zeroed words: the order pass zeroes them
        // each sector's waves in the order of its own weight: split waves, or sector launches (need_merge alone)
        rc = launch_schedule(sX, sZ, sbits, B, c.mX, c.mZ, d->sched.data(), split ? d->merge.data() : nullptr, sectors,
                             &pm, &perm_sectors, st, method, d->gbar.data());
        if (rc) return rc;
        perm = pm;
        zeroed = split;
    }
    // QEC_OPT_LIGHT_MEMO: the outcome table of this launch's key (p', N, stop).  A new key fills it first, on this
    // stream, with the decoder's own kernels (no synchronisation); while the stream is being captured a cold key
    // is not filled and the launch runs without the table.
    const uint16_t* memo = nullptr;
    const float pp = 2.0f / 3.0f * p;
    if (d->light_memo && !d->phase_stats && d->memo_tab.capacity() > 0 && stop != QEC_STOP_SYNDROME && q == nullptr &&
        maxIter >= 2 && maxIter <= 0xFFFF && pp > 0.0f && pp < 1.0f) {
        uint32_t key[3] = {0, (uint32_t)maxIter, (uint32_t)stop};
        std::memcpy(&key[0], &pp, sizeof(uint32_t));
        if (d->memo_valid && std::memcmp(key, d->memo_key, sizeof key) == 0) {
            memo = d->memo_tab.data();
        } else if (!capturing(st)) {
            d->memo_valid = false;
            if ((rc = launch_memo_fill(d->variant, c, p, maxIter, stop, hp, d->memo_tab.data(), d->memo_ws.data(), st)))
                return rc;
            std::memcpy(d->memo_key, key, sizeof key);
            d->memo_valid = true;
            memo = d->memo_tab.data();
        }
    }
    rc = launch_decode(d->variant, c, sX, sZ, sbits, B, p, maxIter, stop, eX, eZ, flags, rec, iters, q, hp, perm,
                       split_opt, need_merge ? d->merge.data() : nullptr, zeroed, st, rec_stride, perm_sectors,
                       ws_done(d, st), memo);
    if (rc) return rc;
    d->last_path |= (perm ? QEC_PATH_ORDERED : 0) | (perm && perm_sectors ? QEC_PATH_SECTOR_ORDER : 0) |
                    (split ? QEC_PATH_SPLIT_WAVES : 0) | (need_merge && !split ? QEC_PATH_SECTOR_LAUNCHES : 0);
    return ws_release(d, st, true);
}

const int32_t* syndrome_table(const qec_decoder* d)
{
    return d->engine == QEC_ENGINE_SPARSE ? sparse_plan_chkvar(d->sparse) : nullptr;
}

const int32_t* variable_table(const qec_decoder* d)
{
    return d->engine == QEC_ENGINE_SPARSE ? sparse_plan_varedge(d->sparse) : nullptr;
}

int check_decode_args(const qec_decoder* d, const void* sX, const void* sZ, size_t B, int stop)
{
    if (!d) return fail(QEC_ERR_ARG, "decode: null decoder");
    if (stop < QEC_STOP_REF || stop > QEC_STOP_SYNDROME) return fail(QEC_ERR_ARG, "decode: unknown stop rule");
    if (B && (!sX || !sZ)) return fail(QEC_ERR_ARG, "decode: null syndrome buffer");
    if (B > (size_t)1 << 40) return fail(QEC_ERR_ARG, "decode: batch too large");
    return QEC_OK;
}

int single_device_only(const qec_decoder* d, const char* what)
{
    if (d->cpu) return fail(QEC_ERR_UNSUPPORTED, std::string(what) + ": the CPU engine has no device buffers");
    if (!d->parts.empty())
        return fail(QEC_ERR_ARG, std::string(what) + ": device buffers live on one GPU; call it on a part "
                                                     "(qec_decoder_part) of a multi-device decoder");
    return QEC_OK;
}

// ---- OSD stage (QEC_OPT_OSD) ---------------------------------------------------------
// Samples of the compact batch of failures decoded at once: the soft decode's q_final block is
// (mX + mZ) L floats per sample (24 KB for P61), so the q buffer stays within 256 MiB.
size_t osd_chunk(const Code& c)
{
    const size_t per = (size_t)(c.mX + c.mZ) * c.stride() * sizeof(float);
    return std::max<size_t>(256, std::min<size_t>(65536, ((size_t)256 << 20) / std::max<size_t>(per, 1)));
}

int osd_reserve(qec_decoder* d, size_t cnt)
{
    const Code& c = *d->code;
    try {
        d->osX.reserve(cnt * c.mX); d->osZ.reserve(cnt * c.mZ);
        d->oeX.reserve(cnt * c.n); d->oeZ.reserve(cnt * c.n);
        d->ofl.reserve(cnt); d->ofl0.reserve(cnt); d->ofs.reserve(cnt);
        d->oq.reserve(cnt * (size_t)(c.mX + c.mZ) * c.stride());
    } catch (const std::exception& ex) {
        return fail(QEC_ERR_NOMEM, std::string("OSD workspace: ") + ex.what());
    }
    return QEC_OK;
}

// The compact device batch (osX, osZ: syndromes of samples with a failed sector; ofl: their flags):
// soft decode with the existing decode path (fixed stop, osd_iters iterations, final messages), then
// the elimination kernel repairs oeX / oeZ / ofl (and adds the swept sectors to ocnt[2]; `count`: the
// repaired ones to ocnt[1]).  The soft decode's own flags go to a scratch array
// and its launch sequence does not replace the main decode's in QEC_OPT_LAST_PATH.
int osd_compact_dev(qec_decoder* d, long long cnt, float p, bool count, hipStream_t st)
{
    const int path = d->last_path;
    d->relay_hold = true;  // the soft decode is plain min-sum (or the product rule), whatever relay tables the handle has
    int rc = dispatch_decode(d, d->osX.data(), d->osZ.data(), cnt, p, d->osd_iters, QEC_STOP_FIXED, d->oeX.data(),
                             d->oeZ.data(), d->ofs.data(), nullptr, nullptr, d->oq.data(), st);
    d->relay_hold = false;
    d->last_path = path;
    if (rc) return rc;
    return launch_osd(d->odev, d->osd_sweep, d->osd_order, d->osX.data(), d->osZ.data(), cnt, d->oq.data(), d->oeX.data(),
                      d->oeZ.data(), d->ofl.data(), count ? d->ocnt.data() + 1 : nullptr, d->ocnt.data() + 2, d->osw_dev(), st,
                      d->bp_method == 1);
}

// The whole stage on a decoded host batch of one single-device handle (byte form, or records): find
// the failures, soft decode + OSD of the compact batch in chunks, write the repaired sectors back.
int osd_repair_host(qec_decoder* d, const uint8_t* sX, const uint8_t* sZ, size_t B, float p, uint8_t* eX, uint8_t* eZ,
                    uint8_t* flags, uint8_t* rec)
{
    const Code& c = *d->code;
    const int n = c.n, nb = (n + 7) / 8;
    const size_t recB = 2 * (size_t)nb + 1, qn = (size_t)(c.mX + c.mZ) * c.stride();
    if (!d->cpu && !d->odev) return fail(QEC_ERR_UNSUPPORTED, d->osd_why);
    d->last_path |= QEC_PATH_OSD;
    std::vector<size_t> failed;
    for (size_t b = 0; b < B; ++b)
        if ((rec ? rec[b * recB + 2 * nb] : flags[b]) & QEC_SYNDROME_FAIL_XZ) failed.push_back(b);
    const size_t CH = osd_chunk(c);
    std::vector<uint8_t> cX, cZ, cEX, cEZ, cF, cF0, cFs;
    std::vector<float> cq;
    for (size_t lo = 0; lo < failed.size(); lo += CH) {
        const size_t cnt = std::min(CH, failed.size() - lo);
        cX.resize(cnt * c.mX); cZ.resize(cnt * c.mZ); cEX.resize(cnt * n); cEZ.resize(cnt * n);
        cF.resize(cnt); cF0.resize(cnt);
        for (size_t i = 0; i < cnt; ++i) {
            const size_t b = failed[lo + i];
            std::memcpy(&cX[i * c.mX], sX + b * c.mX, c.mX);
            std::memcpy(&cZ[i * c.mZ], sZ + b * c.mZ, c.mZ);
            cF[i] = cF0[i] = rec ? rec[b * recB + 2 * nb] : flags[b];
        }
        if (d->cpu) {
            cq.resize(cnt * qn);
            cFs.resize(cnt);
            const int rc = cpu_decode_batch(d->cpu, cX.data(), cZ.data(), (long long)cnt, p, d->osd_iters, QEC_STOP_FIXED,
                                            cEX.data(), cEZ.data(), cFs.data(), nullptr, nullptr, cq.data(), 0,
                                            false, d->prior_host(), d->correlated, d->cond_host(), d->bp_schedule,
                                            d->minsum(), d->llr_host(), nullptr, 0, 0, nullptr,  // never the relay
                                            d->bp_method == 1 && d->minsum_schedule == 1);
            if (rc) return rc;
            long long swept = 0;
            osd_host_batch(*d->oplan, cX.data(), cZ.data(), (long long)cnt, cq.data(), cEX.data(), cEZ.data(), cF.data(), 0,
                           d->osd_order, &swept, d->osw_host(), d->bp_method == 1);
            d->osd_cs_sectors += (unsigned long long)swept;
        } else {
            hipStream_t st = d->stream;
            int rc = osd_reserve(d, cnt);
            if (rc) return rc;
            QEC_HIP_CHECK(hipMemcpyAsync(d->osX.data(), cX.data(), cnt * c.mX, hipMemcpyHostToDevice, st));
            QEC_HIP_CHECK(hipMemcpyAsync(d->osZ.data(), cZ.data(), cnt * c.mZ, hipMemcpyHostToDevice, st));
            QEC_HIP_CHECK(hipMemcpyAsync(d->ofl.data(), cF.data(), cnt, hipMemcpyHostToDevice, st));
            QEC_HIP_CHECK(hipMemsetAsync(d->ocnt.data() + 2, 0, sizeof(uint32_t), st));
            if ((rc = osd_compact_dev(d, (long long)cnt, p, false, st))) return rc;
            uint32_t swept = 0;
            QEC_HIP_CHECK(hipMemcpyAsync(&swept, d->ocnt.data() + 2, sizeof swept, hipMemcpyDeviceToHost, st));
            QEC_HIP_CHECK(hipMemcpyAsync(cEX.data(), d->oeX.data(), cnt * n, hipMemcpyDeviceToHost, st));
            QEC_HIP_CHECK(hipMemcpyAsync(cEZ.data(), d->oeZ.data(), cnt * n, hipMemcpyDeviceToHost, st));
            QEC_HIP_CHECK(hipMemcpyAsync(cF.data(), d->ofl.data(), cnt, hipMemcpyDeviceToHost, st));
            QEC_HIP_CHECK(hipStreamSynchronize(st));
            d->osd_cs_sectors += swept;
        }
        for (size_t i = 0; i < cnt; ++i) {
            const size_t b = failed[lo + i];
            const uint8_t fixed = cF0[i] & (uint8_t)~cF[i];  // fail bits the stage cleared
            for (int sec = 0; sec < 2; ++sec) {
                if (!(fixed & (sec ? QEC_SYNDROME_FAIL_Z : QEC_SYNDROME_FAIL_X))) continue;
                ++d->osd_sectors;
                const uint8_t* e = (sec ? cEZ.data() : cEX.data()) + i * n;
                if (rec) {
                    uint8_t* o = rec + b * recB + (size_t)sec * nb;
                    std::memset(o, 0, nb);
                    for (int v = 0; v < n; ++v) o[v >> 3] |= (uint8_t)((e[v] & 1) << (v & 7));
                } else {
                    std::memcpy((sec ? eZ : eX) + b * n, e, n);
                }
            }
            if (rec) rec[b * recB + 2 * nb] = cF[i];
            else flags[b] = cF[i];
        }
    }
    return QEC_OK;
}

// The stage on the packed decision records of a device batch (the Monte-Carlo pipeline; syndromes as
// bit rows or bytes, records at row stride rstride), on the handle's stream: the failed records'
// indices, then per chunk of them gather, soft decode + OSD, write-back.  Reads the list length back
// once (one synchronisation per batch).
int osd_stage_records(qec_decoder* d, const uint8_t* sX, const uint8_t* sZ, bool bits, long long B, float p,
                      uint8_t* rec, int rstride)
{
    const Code& c = *d->code;
    hipStream_t st = d->stream;
    if (!d->odev) return fail(QEC_ERR_UNSUPPORTED, d->osd_why);
    if (B <= 0) return QEC_OK;
    try {
        d->olist.reserve((size_t)B);
        d->ocnt_h.reserve(3);
    } catch (const std::exception& ex) {
        return fail(QEC_ERR_NOMEM, std::string("OSD workspace: ") + ex.what());
    }
    QEC_HIP_CHECK(hipMemsetAsync(d->ocnt.data(), 0, sizeof(uint32_t), st));
    int rc = launch_osd_collect(rec, rstride, c.n, B, d->olist.data(), d->ocnt.data(), st);
    if (rc) return rc;
    QEC_HIP_CHECK(hipMemcpyAsync(d->ocnt_h.data(), d->ocnt.data(), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    QEC_HIP_CHECK(hipStreamSynchronize(st));
    const size_t total = d->ocnt_h[0];
    d->last_path |= QEC_PATH_OSD;
    if (total == 0) return QEC_OK;
    const size_t CH = osd_chunk(c);
    if ((rc = osd_reserve(d, std::min(CH, total)))) return rc;
    for (size_t lo = 0; lo < total; lo += CH) {
        const long long cnt = (long long)std::min(CH, total - lo);
        const int32_t* list = d->olist.data() + lo;
        if ((rc = launch_osd_gather(list, cnt, sX, sZ, bits, c.mX, c.mZ, rec, rstride, c.n, d->osX.data(), d->osZ.data(),
                                    d->ofl.data(), d->ofl0.data(), st)) ||
            (rc = osd_compact_dev(d, cnt, p, true, st)) ||
            (rc = launch_osd_scatter(list, cnt, d->oeX.data(), d->oeZ.data(), d->ofl.data(), d->ofl0.data(), c.n, rec,
                                     rstride, st)))
            return rc;
    }
    return QEC_OK;
}

// QEC_OPT_OSD_SECTORS and QEC_OPT_OSD_CS_SECTORS of a device pipeline call: the kernel's counters,
// zeroed before the call's first batch and read after its last (the stream is synchronised then).
int osd_count_begin(qec_decoder* d)
{
    d->osd_sectors = 0;
    d->osd_cs_sectors = 0;
    if (d->osd && d->odev) QEC_HIP_CHECK(hipMemsetAsync(d->ocnt.data() + 1, 0, 2 * sizeof(uint32_t), d->stream));
    return QEC_OK;
}
int osd_count_end(qec_decoder* d)
{
    if (!d->osd || !d->odev) return QEC_OK;
    try {
        d->ocnt_h.reserve(3);
    } catch (const std::exception& ex) {
        return fail(QEC_ERR_NOMEM, std::string("OSD workspace: ") + ex.what());
    }
    QEC_HIP_CHECK(hipMemcpyAsync(d->ocnt_h.data() + 1, d->ocnt.data() + 1, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, d->stream));
    QEC_HIP_CHECK(hipStreamSynchronize(d->stream));
    d->osd_sectors = d->ocnt_h[1];
    d->osd_cs_sectors = d->ocnt_h[2];
    return QEC_OK;
}

// Host-buffer decode of one single-device handle (synchronous): stage, decode, copy back.
int decode_host(qec_decoder* d, const uint8_t* sX, const uint8_t* sZ, size_t B, float p, int maxIter, int stop,
                uint8_t* eX, uint8_t* eZ, uint8_t* flags, uint8_t* rec, int32_t* iters, float* q, uint8_t* fX = nullptr,
                uint8_t* fZ = nullptr)
{
    d->osd_sectors = 0;
    d->osd_cs_sectors = 0;
    if (B == 0) return QEC_OK;
    if (d->cpu) {
        const int rc = cpu_decode_batch(d->cpu, sX, sZ, (long long)B, p, maxIter, stop, eX, eZ, flags, rec, iters, q, 0,
                                        d->hard_paths && d->near_hard, d->prior_host(), d->correlated, d->cond_host(),
                                        d->bp_schedule, d->minsum(), d->llr_host(), d->relay_host(), d->relay_legs,
                                        d->relay_solutions, d->relay_w_host(), d->layered_on(), d->mu_host(), fX, fZ);
        d->last_path = (d->correlated ? QEC_PATH_CORRELATED : 0) | (d->bp_schedule || d->layered_on() ? QEC_PATH_SERIAL : 0) |
                       (d->bp_method ? QEC_PATH_MINSUM : 0) | (d->relay_on() ? QEC_PATH_RELAY : 0) |
                       (d->soft_on() ? QEC_PATH_SOFT : 0);
        return rc || !d->osd ? rc : osd_repair_host(d, sX, sZ, B, p, eX, eZ, flags, rec);
    }
    QEC_DEVICE_SCOPE(d->device);
    const Code& c = *d->code;
    const size_t qn = (size_t)(c.mX + c.mZ) * c.stride();
    const size_t recB = 2 * (size_t)((c.n + 7) / 8) + 1;
    hipStream_t st = d->stream;
    try {
        d->sX.reserve(B * c.mX); d->sZ.reserve(B * c.mZ);
        if (rec) d->rec.reserve(B * recB);
        else { d->eX.reserve(B * c.n); d->eZ.reserve(B * c.n); d->flags.reserve(B); }
        if (iters) d->iters.reserve(2 * B);
        if (q) d->q.reserve(B * qn);
        if (fX) d->fX.reserve(B * c.mX);
        if (fZ) d->fZ.reserve(B * c.mZ);
    } catch (const std::exception& ex) {
        return fail(QEC_ERR_HIP, std::string("device staging allocation: ") + ex.what());
    }
    QEC_HIP_CHECK(hipMemcpyAsync(d->sX.data(), sX, B * c.mX, hipMemcpyHostToDevice, st));
    QEC_HIP_CHECK(hipMemcpyAsync(d->sZ.data(), sZ, B * c.mZ, hipMemcpyHostToDevice, st));
    // the sparse engine's packed path stages its byte outputs in eX/eZ/flags (dispatch_decode)
    int rc = dispatch_decode(d, d->sX.data(), d->sZ.data(), (long long)B, p, maxIter, stop, rec ? nullptr : d->eX.data(),
                             rec ? nullptr : d->eZ.data(), rec ? nullptr : d->flags.data(), rec ? d->rec.data() : nullptr,
                             iters ? d->iters.data() : nullptr, q ? d->q.data() : nullptr, st, false, 0,
                             fX ? d->fX.data() : nullptr, fZ ? d->fZ.data() : nullptr);
    if (rc) return rc;
    if (fX) QEC_HIP_CHECK(hipMemcpyAsync(fX, d->fX.data(), B * c.mX, hipMemcpyDeviceToHost, st));
    if (fZ) QEC_HIP_CHECK(hipMemcpyAsync(fZ, d->fZ.data(), B * c.mZ, hipMemcpyDeviceToHost, st));
    if (rec) {
        QEC_HIP_CHECK(hipMemcpyAsync(rec, d->rec.data(), B * recB, hipMemcpyDeviceToHost, st));
    } else {
        QEC_HIP_CHECK(hipMemcpyAsync(eX, d->eX.data(), B * c.n, hipMemcpyDeviceToHost, st));
        QEC_HIP_CHECK(hipMemcpyAsync(eZ, d->eZ.data(), B * c.n, hipMemcpyDeviceToHost, st));
        QEC_HIP_CHECK(hipMemcpyAsync(flags, d->flags.data(), B, hipMemcpyDeviceToHost, st));
    }
    if (iters) QEC_HIP_CHECK(hipMemcpyAsync(iters, d->iters.data(), 2 * B * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (q) QEC_HIP_CHECK(hipMemcpyAsync(q, d->q.data(), B * qn * sizeof(float), hipMemcpyDeviceToHost, st));
    QEC_HIP_CHECK(hipStreamSynchronize(st));
    return d->osd ? osd_repair_host(d, sX, sZ, B, p, eX, eZ, flags, rec) : QEC_OK;
}

// Host-buffer decode on every part of a handle: contiguous shards, one host thread per part
// (the reference's sample-parallel loop, DecoderCPU.h:419-438, across devices).
int decode_host_parts(qec_decoder* d, const uint8_t* sX, const uint8_t* sZ, size_t B, float p, int maxIter, int stop,
                      uint8_t* eX, uint8_t* eZ, uint8_t* flags, uint8_t* rec, int32_t* iters, float* q,
                      uint8_t* fX = nullptr, uint8_t* fZ = nullptr)
{
    const std::vector<qec_decoder*> parts = parts_of(d);
    if (parts.size() == 1)
        return decode_host(parts[0], sX, sZ, B, p, maxIter, stop, eX, eZ, flags, rec, iters, q, fX, fZ);
    const Code& c = *d->code;
    const size_t qn = (size_t)(c.mX + c.mZ) * c.stride();
    const size_t recB = 2 * (size_t)((c.n + 7) / 8) + 1;
    const int np = (int)parts.size();
    std::vector<int> rcs(np, QEC_OK);
    std::vector<std::string> errs(np);
    std::vector<std::thread> th;
    for (int k = 0; k < np; ++k) {
        const size_t lo = (size_t)shard_lo((long long)B, k, np), hi = (size_t)shard_lo((long long)B, k + 1, np);
        th.emplace_back([&, k, lo, hi] {
            rcs[k] = decode_host(parts[k], sX + lo * c.mX, sZ + lo * c.mZ, hi - lo, p, maxIter, stop,
                                 eX ? eX + lo * c.n : nullptr, eZ ? eZ + lo * c.n : nullptr, flags ? flags + lo : nullptr,
                                 rec ? rec + lo * recB : nullptr, iters ? iters + 2 * lo : nullptr, q ? q + lo * qn : nullptr,
                                 fX ? fX + lo * c.mX : nullptr, fZ ? fZ + lo * c.mZ : nullptr);
            if (rcs[k]) errs[k] = last_error_cstr();
        });
    }
    for (auto& t : th) t.join();
    for (int k = 0; k < np; ++k)
        if (rcs[k]) return fail(rcs[k], "part " + std::to_string(k) + ": " + errs[k]);
    return QEC_OK;
}

}  // namespace

extern "C" {

int qec_decode_batch_dev(qec_decoder* d, const uint8_t* sX, const uint8_t* sZ, size_t B, float p, int maxIter,
                         int stop, uint8_t* eX, uint8_t* eZ, uint8_t* flags, int32_t* iters, float* q, void* stream)
{
    int rc = check_decode_args(d, sX, sZ, B, stop);
    if (rc || (rc = single_device_only(d, "qec_decode_batch_dev"))) return rc;
    if (B && (!eX || !eZ || !flags)) return fail(QEC_ERR_ARG, "decode: null output buffer");
    QEC_DEVICE_SCOPE(d->device);
    return dispatch_decode(d, sX, sZ, (long long)B, p, maxIter, stop, eX, eZ, flags, nullptr, iters, q,
                           static_cast<hipStream_t>(stream));
}

int qec_decode_batch_packed_dev(qec_decoder* d, const uint8_t* sX, const uint8_t* sZ, size_t B, float p, int maxIter,
                                int stop, uint8_t* records, int32_t* iters, float* q, void* stream)
{
    int rc = check_decode_args(d, sX, sZ, B, stop);
    if (rc || (rc = single_device_only(d, "qec_decode_batch_packed_dev"))) return rc;
    if (B && !records) return fail(QEC_ERR_ARG, "decode: null record buffer");
    QEC_DEVICE_SCOPE(d->device);
    return dispatch_decode(d, sX, sZ, (long long)B, p, maxIter, stop, nullptr, nullptr, nullptr, records, iters, q,
                           static_cast<hipStream_t>(stream));
}

int qec_decode_bits_packed_dev(qec_decoder* d, const uint32_t* sX, const uint32_t* sZ, size_t B, float p, int maxIter,
                               int stop, uint8_t* records, int32_t* iters, float* q, void* stream)
{
    int rc = check_decode_args(d, sX, sZ, B, stop);
    if (rc || (rc = single_device_only(d, "qec_decode_bits_packed_dev"))) return rc;
    if (B && !records) return fail(QEC_ERR_ARG, "decode: null record buffer");
    if (d->engine == QEC_ENGINE_SPARSE)
        return fail(QEC_ERR_UNSUPPORTED, "qec_decode_bits_packed_dev: bit-row syndromes need the wave-circulant engine");
    QEC_DEVICE_SCOPE(d->device);
    return dispatch_decode(d, reinterpret_cast<const uint8_t*>(sX), reinterpret_cast<const uint8_t*>(sZ), (long long)B, p,
                           maxIter, stop, nullptr, nullptr, nullptr, records, iters, q, static_cast<hipStream_t>(stream),
                           true);
}

int qec_decode_batch(qec_decoder* d, const uint8_t* sX, const uint8_t* sZ, size_t B, float p, int maxIter, int stop,
                     uint8_t* eX, uint8_t* eZ, uint8_t* flags, int32_t* iters, float* q)
{
    int rc = check_decode_args(d, sX, sZ, B, stop);
    if (rc) return rc;
    if (B && (!eX || !eZ || !flags)) return fail(QEC_ERR_ARG, "decode: null output buffer");
    return decode_host_parts(d, sX, sZ, B, p, maxIter, stop, eX, eZ, flags, nullptr, iters, q);
}

int qec_decode_batch_soft(qec_decoder* d, const uint8_t* sX, const uint8_t* sZ, size_t B, float p, int maxIter, int stop,
                          uint8_t* eX, uint8_t* eZ, uint8_t* fX, uint8_t* fZ, uint8_t* flags, int32_t* iters, float* q)
{
    int rc = check_decode_args(d, sX, sZ, B, stop);
    if (rc) return rc;
    if (B && (!eX || !eZ || !flags)) return fail(QEC_ERR_ARG, "decode: null output buffer");
    if (d->bp_method != 1) return fail(QEC_ERR_UNSUPPORTED, "qec_decode_batch_soft: a min-sum call; set QEC_OPT_BP_METHOD to 1");
    return decode_host_parts(d, sX, sZ, B, p, maxIter, stop, eX, eZ, flags, nullptr, iters, q, fX, fZ);
}

int qec_decode_batch_soft_dev(qec_decoder* d, const uint8_t* sX, const uint8_t* sZ, size_t B, float p, int maxIter,
                              int stop, uint8_t* eX, uint8_t* eZ, uint8_t* fX, uint8_t* fZ, uint8_t* flags, int32_t* iters,
                              float* q, void* stream)
{
    int rc = check_decode_args(d, sX, sZ, B, stop);
    if (rc || (rc = single_device_only(d, "qec_decode_batch_soft_dev"))) return rc;
    if (B && (!eX || !eZ || !flags)) return fail(QEC_ERR_ARG, "decode: null output buffer");
    if (d->bp_method != 1)
        return fail(QEC_ERR_UNSUPPORTED, "qec_decode_batch_soft_dev: a min-sum call; set QEC_OPT_BP_METHOD to 1");
    QEC_DEVICE_SCOPE(d->device);
    return dispatch_decode(d, sX, sZ, (long long)B, p, maxIter, stop, eX, eZ, flags, nullptr, iters, q,
                           static_cast<hipStream_t>(stream), false, 0, fX, fZ);
}

int qec_flip_syndrome_dev(qec_decoder* d, uint64_t seed, uint64_t start, size_t B, uint8_t* sX, uint8_t* sZ, uint8_t* fX,
                          uint8_t* fZ, void* stream)
{
    if (!d || (B && (!sX || !sZ))) return fail(QEC_ERR_ARG, "qec_flip_syndrome_dev: bad argument");
    int rc = single_device_only(d, "qec_flip_syndrome_dev");
    if (rc) return rc;
    if (!d->has_syn)
        return fail(QEC_ERR_ARG, "qec_flip_syndrome_dev: the decoder has no syndrome priors (qec_decoder_set_syndrome_priors)");
    QEC_DEVICE_SCOPE(d->device);
    return launch_flip_syndrome(seed, start, (long long)B, d->code->mX, d->code->mZ, d->synq_dev(), sX, sZ, fX, fZ,
                                static_cast<hipStream_t>(stream));
}

int qec_decode_batch_packed(qec_decoder* d, const uint8_t* sX, const uint8_t* sZ, size_t B, float p, int maxIter,
                            int stop, uint8_t* records, int32_t* iters)
{
    int rc = check_decode_args(d, sX, sZ, B, stop);
    if (rc) return rc;
    if (B && !records) return fail(QEC_ERR_ARG, "decode: null record buffer");
    return decode_host_parts(d, sX, sZ, B, p, maxIter, stop, nullptr, nullptr, nullptr, records, iters, nullptr);
}

int qec_sample_fixed_weight(uint32_t seed, int W, size_t count, int n, uint8_t* x, uint8_t* z)
{
    if (n <= 0 || W < 0 || (count && (!x || !z))) return fail(QEC_ERR_ARG, "qec_sample_fixed_weight: bad argument");
    Mt19937 g(seed);
    std::memset(x, 0, count * n);
    std::memset(z, 0, count * n);
    for (size_t c = 0; c < count; ++c)
        for (int w = 0; w < W; ++w) {
            const uint32_t index = g.msvc_uniform((uint32_t)n);
            const uint32_t type = g.msvc_uniform(3u);  // x = 0, y = 1, z = 2
            if (type == 0 || type == 1) x[c * n + index] = 1;
            if (type == 2 || type == 1) z[c * n + index] = 1;
        }
    return QEC_OK;
}

}  // extern "C"

namespace {

// Monte-Carlo workspace of one part for batches of up to B samples (W draws each).
int mc_reserve(qec_decoder* d, size_t B, int W)
{
    const Code& c = *d->code;
    const size_t nb = (size_t)(c.n + 7) / 8;
    try {
        // syndromes as bytes or as bit rows, packed errors at 2 nb or word-aligned rows (mc_batch)
        d->msX.reserve(B * std::max<size_t>(c.mX, 4 * ((c.mX + 31) / 32)));
        d->msZ.reserve(B * std::max<size_t>(c.mZ, 4 * ((c.mZ + 31) / 32)));
        d->merrp.reserve(B * 4 * ((2 * nb + 3) / 4)); d->mrec.reserve(B * 4 * ((2 * nb + 1 + 3) / 4));
        d->mit.reserve(2 * B);
        if (W > 0) { d->midx.reserve(B * W); d->mtype.reserve(B * W); }
    } catch (const std::exception& ex) {
        return fail(QEC_ERR_HIP, std::string("Monte-Carlo workspace: ") + ex.what());
    }
    return QEC_OK;
}

// errors (source filled in h by the caller) -> syndromes + packed errors -> packed decode ->
// counters, all enqueued on the part's stream
// zero_counters: the call's first batch (the counters start at 0; one memset with the fused
// pipeline's list lengths, enqueued after the host-side preparation, right before the first kernel)
int mc_batch(qec_decoder* d, McArgsHost h, int src, float p, int maxIter, int stop, bool want_iters,
             hipEvent_t ev0, hipEvent_t ev1, bool zero_counters = false)
{
    hipStream_t st = d->stream;
    const Code& c = *d->code;
    h.code = &c;
    h.chkVar = syndrome_table(d);
    h.varEdge = variable_table(d);
    // the depolarising front end hands the wave-circulant engine its syndromes as bit rows and its
    // packed errors at word-aligned rows (72 + 156 instead of 549 + 154 B per P61 sample)
    const bool bits = src == MC_SRC_PHILOX && d->engine != QEC_ENGINE_SPARSE;
    const int nb = (c.n + 7) / 8;
    const int estride = bits ? 4 * ((2 * nb + 3) / 4) : 2 * nb;
    const int padded = 4 * ((2 * nb + 1 + 3) / 4);
    const int rstride = bits && statistics_lane_shape(estride, padded) ? padded : 2 * nb + 1;
    // the fused low-p pipeline (triage.hip: sampler, syndromes, iteration-0 triage and the finished
    // samples' statistics in one kernel; the list-mode decode and the survivors' statistics after it)
    uint32_t pats[4];
    if (!d->osd && bits && stop == QEC_STOP_SYNDROME && want_iters && d->triage != 3 && triage_on(d, p) && maxIter >= 2 &&
        h.B < (1LL << 31) && decode_has_list(d->variant) && mc_fused_supported(c, rstride) &&
        decode_pattern_masks(d->variant, p, pats)) {
        const long long B = h.B;
        int rc = ws_acquire(d, st);
        if (rc) return rc;
        if ((rc = ws_reserve(d->merge, (size_t)B, st, "monte carlo")) ||
            (rc = ws_reserve(d->tlist, 3 * (size_t)B, st, "monte carlo")) ||
            (rc = ws_reserve(d->mpart, (size_t)mc_fused_part_rows() * QEC_MC_NCOUNTERS_ALL, st, "monte carlo")))
            return rc;
        int32_t* lX = d->tlist.data();
        int32_t* lZ = lX + B;
        int32_t* lS = lZ + B;
        uint32_t* cnt = reinterpret_cast<uint32_t*>(d->mcount.data() + QEC_MC_NCOUNTERS_ALL);  // list lengths
        uint32_t* sXp = reinterpret_cast<uint32_t*>(d->msX.data());
        uint32_t* sZp = reinterpret_cast<uint32_t*>(d->msZ.data());
        // the counters (first batch), the list lengths and the partial-sum rows, in one launch
        const int nz = mc_fused_part_rows() * QEC_MC_NCOUNTERS_ALL;
        rc = zero_counters ? launch_zero_words(d->mcount.data(), QEC_MC_NCOUNTERS_ALL + mc_count_u64(), st, d->mpart.data(), nz)
                           : launch_zero_words(d->mcount.data() + QEC_MC_NCOUNTERS_ALL, mc_count_u64(), st, d->mpart.data(), nz);
        if (rc) return rc;
        // the events here are separate records: carried by the kernels (launch_marked) this pipeline ran
        // 1.5-2.4 % slower at p = 0.001 .. 0.005 (profiles/r06/ab/cmp_event_carry.txt)
        if (ev0) QEC_HIP_CHECK(hipEventRecord(ev0, st));
        auto fused = [&](int stage) {
            return launch_mc_fused(c, h.seed, h.start, B, h.p, pats, sXp, sZp, d->mrec.data(), rstride, d->mit.data(),
                                   d->merge.data(), lX, lZ, lS, cnt, d->imp_cols.data(), d->mcount.data(), d->mpart.data(),
                                   stage, st);
        };
        if ((rc = fused(MC_FUSED_SAMPLE))) return rc;
        rc = launch_decode_list(d->variant, c, d->msX.data(), d->msZ.data(), B, p, maxIter, hard_path_bits(d), d->mrec.data(),
                                d->mit.data(), d->merge.data(), lX, lZ, cnt, st, rstride, true, mc_fused_count_stride());
        if (rc) return rc;
        if (ev1) QEC_HIP_CHECK(hipEventRecord(ev1, st));
        if ((rc = fused(MC_FUSED_SURVIVORS))) return rc;
        return ws_release(d, st);
    }
    if (bits) {
        h.sXp = reinterpret_cast<uint32_t*>(d->msX.data());
        h.sZp = reinterpret_cast<uint32_t*>(d->msZ.data());
        h.errp_words = true;
    } else {
        h.sX = d->msX.data(); h.sZ = d->msZ.data();
    }
    h.errp = d->merrp.data();
    if (zero_counters) QEC_HIP_CHECK(hipMemsetAsync(d->mcount.data(), 0, QEC_MC_NCOUNTERS_ALL * sizeof(unsigned long long), st));
    int rc = launch_mc_errors_syndrome(src, h, st);
    if (rc) return rc;
    // syndrome priors: the measurement-error channel on the sampled syndromes (qec_monte_carlo; GetStatistics' draws have
    // no seeded index space and stay as they are)
    if (d->soft_on() && src != MC_SRC_DRAWS &&
        (rc = launch_flip_syndrome(h.seed, h.start, h.B, c.mX, c.mZ, d->synq_dev(), d->msX.data(), d->msZ.data(), nullptr,
                                   nullptr, st)))
        return rc;
    if (ev0) QEC_HIP_CHECK(hipEventRecord(ev0, st));
    // records at word-aligned rows (156 instead of 155 B for P61) on the bit-row path where the lane
    // statistics kernel has that row shape (rstride above: it then reads both arrays a word at a time);
    // every other code keeps the public 2 nb + 1 rows, which the other statistics kernel, the triage
    // and the list-mode decode take as they are
    rc = dispatch_decode(d, d->msX.data(), d->msZ.data(), h.B, p, maxIter, stop, nullptr, nullptr, nullptr,
                         d->mrec.data(), want_iters ? d->mit.data() : nullptr, nullptr, st, bits, rstride);
    if (rc) return rc;
    if (ev1) QEC_HIP_CHECK(hipEventRecord(ev1, st));
    // QEC_OPT_OSD: repair the records of the samples BP left unsatisfied before they are counted
    if (d->osd && (rc = osd_stage_records(d, d->msX.data(), d->msZ.data(), bits, h.B, p, d->mrec.data(), rstride)))
        return rc;
    return launch_statistics_packed(c, d->imp_cols.data(), d->merrp.data(), estride, d->mrec.data(),
                                    want_iters ? d->mit.data() : nullptr, h.B, d->mcount.data(), st, rstride);
}

// Enqueues the counters' copy into the handle's page-locked host buffer (mhost); valid after the
// stream has been synchronised.
int mc_enqueue_counters(qec_decoder* d)
{
    try {
        d->mhost.reserve(QEC_MC_NCOUNTERS_ALL);
    } catch (const std::exception& ex) {
        return fail(QEC_ERR_HIP, std::string("counter staging allocation: ") + ex.what());
    }
    QEC_HIP_CHECK(hipMemcpyAsync(d->mhost.data(), d->mcount.data(), QEC_MC_NCOUNTERS_ALL * sizeof(unsigned long long),
                                 hipMemcpyDeviceToHost, d->stream));
    return QEC_OK;
}

int mc_fetch_counters(qec_decoder* d, unsigned long long* out)
{
    int rc = mc_enqueue_counters(d);
    if (rc) return rc;
    QEC_HIP_CHECK(hipStreamSynchronize(d->stream));
    std::memcpy(out, d->mhost.data(), QEC_MC_NCOUNTERS_ALL * sizeof(unsigned long long));
    return QEC_OK;
}


// qec_monte_carlo on one part: samples [start, start + count), counters left in d->mcount
int monte_carlo_part(qec_decoder* d, uint64_t seed, uint64_t start, uint64_t count, float p, int maxIter, int stop,
                     size_t batch, double* decode_s)
{
    QEC_DEVICE_SCOPE(d->device);
    hipStream_t st = d->stream;
    int rc = mc_reserve(d, (size_t)std::min<uint64_t>(batch, std::max<uint64_t>(count, 1)), 0);
    if (rc || (rc = osd_count_begin(d))) return rc;
    // decode-kernel time from a ring of event pairs: the host waits only on a pair it reuses,
    // kRing batches behind the launches (no per-batch synchronisation)
    constexpr size_t kRing = 32;
    if (d->mc_ev.ev.empty() && (rc = d->mc_ev.make(2 * kRing, hipEventDefault | kEvNoFence))) return rc;  // once per handle
    EventSet& ev = d->mc_ev;
    double dec = 0;
    uint64_t k = 0;
    auto harvest = [&](size_t slot) -> int {
        QEC_HIP_CHECK(hipEventSynchronize(ev.ev[2 * slot + 1]));
        float ms = 0;
        QEC_HIP_CHECK(hipEventElapsedTime(&ms, ev.ev[2 * slot], ev.ev[2 * slot + 1]));
        dec += ms * 1e-3;
        return QEC_OK;
    };
    for (uint64_t base = 0; base < count; base += batch, ++k) {
        const size_t slot = k % kRing;
        if (d->mc_time && k >= kRing && (rc = harvest(slot))) return rc;
        McArgsHost h;
        h.seed = seed; h.start = start + base; h.p = p;
        h.prior = d->prior_dev();
        h.pauli_thr = d->has_channel ? d->dpth.data() : nullptr;
        h.B = (long long)std::min<uint64_t>(batch, count - base);
        // priors set: the independent sampler over them (a Pauli channel: its own sampler); mc_batch then takes
        // the unfused byte-syndrome pipeline
        rc = mc_batch(d, h, d->has_channel ? MC_SRC_PAULI : d->has_priors ? MC_SRC_INDEPENDENT : MC_SRC_PHILOX, p, maxIter, stop, true, d->mc_time ? ev.ev[2 * slot] : nullptr,
                      d->mc_time ? ev.ev[2 * slot + 1] : nullptr, k == 0);
        if (rc) return rc;
    }
    if (k == 0)  // no batch zeroed the counters
        QEC_HIP_CHECK(hipMemsetAsync(d->mcount.data(), 0, QEC_MC_NCOUNTERS_ALL * sizeof(unsigned long long), st));
    // the counters' copy behind the last batch, one synchronisation for the whole run; the remaining
    // event pairs are complete by then (qec_monte_carlo reads the counters from mhost)
    if ((rc = mc_enqueue_counters(d))) return rc;
    QEC_HIP_CHECK(hipStreamSynchronize(st));
    for (uint64_t j = k > kRing ? k - kRing : 0; d->mc_time && j < k; ++j)
        if ((rc = harvest(j % kRing))) return rc;
    *decode_s = dec;
    return osd_count_end(d);
}

// GetStatistics on the CPU engine: the same draws, host syndromes, CPU decode (reference stop
// rule), host counting (DecoderCPU.h:448-521).
int cpu_statistics(qec_decoder* d, int W, long tested, float p, int maxIter, uint32_t seed, qec_stats* out)
{
    const Code& c = *d->code;
    const int n = c.n;
    const long CH = 1 << 14;
    std::vector<uint8_t> x, z, sx, sz, ex, ez, fl, rx(n), rz(n);
    unsigned long long cn[QEC_MC_NCOUNTERS] = {};
    unsigned long long repaired = 0, swept = 0;
    Mt19937 g(seed);
    for (long base = 0; base < tested; base += CH) {
        const long cnt = std::min(CH, tested - base);
        x.assign((size_t)cnt * n, 0);
        z.assign((size_t)cnt * n, 0);
        for (long s = 0; s < cnt; ++s)
            for (int w = 0; w < W; ++w) {
                const uint32_t v = g.msvc_uniform((uint32_t)n), t = g.msvc_uniform(3u);  // DecoderCPU.h:452-457
                if (t == 0 || t == 1) x[(size_t)s * n + v] = 1;
                if (t == 2 || t == 1) z[(size_t)s * n + v] = 1;
            }
        sx.resize((size_t)cnt * c.mX);
        sz.resize((size_t)cnt * c.mZ);
        for (long s = 0; s < cnt; ++s) {
            host_syndrome(c, 0, &x[(size_t)s * n], &sx[(size_t)s * c.mX]);
            host_syndrome(c, 1, &z[(size_t)s * n], &sz[(size_t)s * c.mZ]);
        }
        ex.resize((size_t)cnt * n);
        ez.resize((size_t)cnt * n);
        fl.resize(cnt);
        const int rc = cpu_decode_batch(d->cpu, sx.data(), sz.data(), cnt, p, maxIter, QEC_STOP_REF, ex.data(), ez.data(),
                                        fl.data(), nullptr, nullptr, nullptr, 0, d->hard_paths && d->near_hard,
                                        d->prior_host(), d->correlated, d->cond_host(), d->bp_schedule, d->minsum(),
                                        d->llr_host(), d->relay_host(), d->relay_legs, d->relay_solutions, d->relay_w_host(),
                                        d->layered_on(), d->mu_host());
        if (rc) return rc;
        if (d->osd) {  // the counters describe the repaired estimates
            d->osd_sectors = 0;
            d->osd_cs_sectors = 0;
            const int rc2 = osd_repair_host(d, sx.data(), sz.data(), (size_t)cnt, p, ex.data(), ez.data(), fl.data(), nullptr);
            if (rc2) return rc2;
            repaired += d->osd_sectors;
            swept += d->osd_cs_sectors;
        }
        for (long s = 0; s < cnt; ++s) {
            bool ax = false, az = false;
            for (int v = 0; v < n; ++v) {
                ax |= x[(size_t)s * n + v] != 0;
                az |= z[(size_t)s * n + v] != 0;
            }
            cn[QEC_MC_WITHX] += ax;
            cn[QEC_MC_WITHZ] += az;
            const bool dEX = fl[s] & QEC_SYNDROME_FAIL_X, dEZ = fl[s] & QEC_SYNDROME_FAIL_Z;
            cn[QEC_MC_SYNX] += dEX;
            cn[QEC_MC_SYNZ] += dEZ;
            if (!(dEX || dEZ)) {
                for (int v = 0; v < n; ++v) {
                    rx[v] = x[(size_t)s * n + v] ^ ex[(size_t)s * n + v];
                    rz[v] = z[(size_t)s * n + v] ^ ez[(size_t)s * n + v];
                }
                ++cn[host_check_logical(c, rx.data(), rz.data()) ? QEC_MC_LOGICAL : QEC_MC_CORRECTED];
            }
            cn[QEC_MC_CONVX] += (fl[s] & QEC_CONVERGENCE_FAIL_X) != 0;
            cn[QEC_MC_CONVZ] += (fl[s] & QEC_CONVERGENCE_FAIL_Z) != 0;
        }
    }
    d->osd_sectors = repaired;
    d->osd_cs_sectors = swept;
    d->last_path = (d->osd ? QEC_PATH_OSD : 0) | (d->correlated ? QEC_PATH_CORRELATED : 0) |
                   (d->bp_schedule || d->layered_on() ? QEC_PATH_SERIAL : 0) | (d->bp_method ? QEC_PATH_MINSUM : 0) |
                   (d->relay_on() ? QEC_PATH_RELAY : 0) | (d->soft_on() ? QEC_PATH_SOFT : 0);
    std::memset(out, 0, sizeof *out);
    out->randSeed = seed;
    out->numErrorsTested = (uint32_t)tested;
    out->numXErrorsTested = (uint32_t)cn[QEC_MC_WITHX];
    out->numZErrorsTested = (uint32_t)cn[QEC_MC_WITHZ];
    out->errorWeight = (uint32_t)W;
    out->corrected = (uint32_t)cn[QEC_MC_CORRECTED];
    out->syndromeErrorsX = (uint32_t)cn[QEC_MC_SYNX];
    out->syndromeErrorsZ = (uint32_t)cn[QEC_MC_SYNZ];
    out->logicalErrors = (uint32_t)cn[QEC_MC_LOGICAL];
    out->convergenceFailX = (uint32_t)cn[QEC_MC_CONVX];
    out->convergenceFailZ = (uint32_t)cn[QEC_MC_CONVZ];
    return QEC_OK;
}

}  // namespace

extern "C" {

// GetStatistics (DecoderCPU.h:392-530).  The errors are the reference's: W (index, type) draws
// per sample from one mt19937(seed) stream through VS2015's uniform_int_distribution, drawn on
// the host in sample order (the stream is sequential), into a double-buffered pinned chunk so the
// next chunk is drawn while the devices work on this one.  Each chunk is sharded contiguously
// over the decoder's parts; on each device: errors from the draws + syndromes + packed errors
// (one fused launch), decode (reference stop rule) to packed records, I-P check and counters.
// The counters do not depend on the sample order, so the per-device sums add up exactly.
int qec_get_statistics(qec_decoder* d, int W, int numErrors, float p, int maxIter, uint32_t seed, int nThreads,
                       qec_stats* out)
{
    if (!d || !out || numErrors < 0 || W < 0) return fail(QEC_ERR_ARG, "qec_get_statistics: bad argument");
    const Code& c = *d->code;
    if (c.imp.empty()) return fail(QEC_ERR_UNSUPPORTED, "qec_get_statistics: code has no I-P matrix for the logical check");
    if (nThreads < 1) nThreads = 1;
    const auto t0 = std::chrono::high_resolution_clock::now();
    const long tested = (long)(numErrors / nThreads) * nThreads;  // DecoderCPU.h:426,527
    if (d->cpu) {
        const int rc = cpu_statistics(d, W, tested, p, maxIter, seed, out);
        out->durationMicroSeconds = std::chrono::duration_cast<std::chrono::microseconds>(
                                        std::chrono::high_resolution_clock::now() - t0).count();
        return rc;
    }
    const long CH = 1 << 16;
    const int n = c.n;
    const std::vector<qec_decoder*> parts = parts_of(d);
    const int np = (int)parts.size();
    const long cap = std::max<long>(1, (std::min<long>(CH, std::max<long>(tested, 1)) + np - 1) / np);
    std::vector<EventSet> consumed(2 * np);  // [buffer][part]: the part's copy out of the pinned buffer is done
    for (int j = 0; j < np; ++j) {
        QEC_DEVICE_SCOPE(parts[j]->device);
        int rc = mc_reserve(parts[j], (size_t)cap, W);
        if (rc || (rc = osd_count_begin(parts[j]))) return rc;
        QEC_HIP_CHECK(hipMemsetAsync(parts[j]->mcount.data(), 0, QEC_MC_NCOUNTERS_ALL * sizeof(unsigned long long),
                                     parts[j]->stream));
        for (int k = 0; k < 2; ++k)
            if ((rc = consumed[k * np + j].make(1, hipEventDisableTiming))) return rc;
    }
    const size_t draws = (size_t)std::min<long>(CH, std::max<long>(tested, 1)) * std::max(W, 1);
    PinnedArray<int32_t> hidx[2];
    PinnedArray<uint8_t> htype[2];
    try {
        for (int k = 0; k < 2; ++k) { hidx[k].reserve(draws); htype[k].reserve(draws); }
    } catch (const std::exception& ex) {
        return fail(QEC_ERR_HIP, std::string("qec_get_statistics: ") + ex.what());
    }
    Mt19937 g(seed);
    long chunk = 0;
    for (long base = 0; base < tested; base += CH, ++chunk) {
        const int k = (int)(chunk & 1);
        const long cnt = std::min(CH, tested - base);
        if (chunk >= 2)
            for (int j = 0; j < np; ++j) QEC_HIP_CHECK(hipEventSynchronize(consumed[k * np + j].ev[0]));
        for (long s = 0; s < cnt; ++s)
            for (int w = 0; w < W; ++w) {
                hidx[k][s * W + w] = (int32_t)g.msvc_uniform((uint32_t)n);  // index, then type (DecoderCPU.h:452-454)
                htype[k][s * W + w] = (uint8_t)g.msvc_uniform(3u);
            }
        for (int j = 0; j < np; ++j) {
            qec_decoder* pd = parts[j];
            const long lo = (long)shard_lo(cnt, j, np), hi = (long)shard_lo(cnt, j + 1, np);
            if (hi == lo) continue;
            QEC_DEVICE_SCOPE(pd->device);
            hipStream_t st = pd->stream;
            if (W > 0) {
                QEC_HIP_CHECK(hipMemcpyAsync(pd->midx.data(), hidx[k].data() + (size_t)lo * W,
                                             (size_t)(hi - lo) * W * sizeof(int32_t), hipMemcpyHostToDevice, st));
                QEC_HIP_CHECK(hipMemcpyAsync(pd->mtype.data(), htype[k].data() + (size_t)lo * W, (size_t)(hi - lo) * W,
                                             hipMemcpyHostToDevice, st));
            }
            QEC_HIP_CHECK(hipEventRecord(consumed[k * np + j].ev[0], st));
            McArgsHost h;
            h.idx = pd->midx.data(); h.type = pd->mtype.data(); h.W = W;
            h.B = hi - lo;
            const int rc = mc_batch(pd, h, MC_SRC_DRAWS, p, maxIter, QEC_STOP_REF, false, nullptr, nullptr);
            if (rc) return rc;
        }
    }
    unsigned long long cn[QEC_MC_NCOUNTERS_ALL] = {};
    for (qec_decoder* pd : parts) {
        QEC_DEVICE_SCOPE(pd->device);
        unsigned long long part[QEC_MC_NCOUNTERS_ALL];
        int rc = mc_fetch_counters(pd, part);
        if (rc || (rc = osd_count_end(pd))) return rc;
        for (int k = 0; k < QEC_MC_NCOUNTERS_ALL; ++k) cn[k] += part[k];
    }
    const auto t1 = std::chrono::high_resolution_clock::now();
    std::memset(out, 0, sizeof *out);
    out->randSeed = seed;
    out->numErrorsTested = (uint32_t)tested;
    out->numXErrorsTested = (uint32_t)cn[QEC_MC_WITHX];
    out->numZErrorsTested = (uint32_t)cn[QEC_MC_WITHZ];
    out->errorWeight = (uint32_t)W;
    out->corrected = (uint32_t)cn[QEC_MC_CORRECTED];
    out->syndromeErrorsX = (uint32_t)cn[QEC_MC_SYNX];
    out->syndromeErrorsZ = (uint32_t)cn[QEC_MC_SYNZ];
    out->logicalErrors = (uint32_t)cn[QEC_MC_LOGICAL];
    out->convergenceFailX = (uint32_t)cn[QEC_MC_CONVX];
    out->convergenceFailZ = (uint32_t)cn[QEC_MC_CONVZ];
    out->durationMicroSeconds = std::chrono::duration_cast<std::chrono::microseconds>(t1 - t0).count();
    return QEC_OK;
}

int qec_monte_carlo(qec_decoder* d, uint64_t seed, uint64_t start, uint64_t count, float p, int maxIter, int stop,
                    size_t batch, qec_mc_result* out)
{
    if (!d || !out || (stop < QEC_STOP_REF || stop > QEC_STOP_SYNDROME)) return fail(QEC_ERR_ARG, "qec_monte_carlo: bad argument");
    if (d->cpu) return fail(QEC_ERR_UNSUPPORTED, "qec_monte_carlo: a device pipeline; the CPU engine has GetStatistics");
    const Code& c = *d->code;
    if (c.imp.empty()) return fail(QEC_ERR_UNSUPPORTED, "qec_monte_carlo: code has no I-P matrix for the logical check");
    if (batch == 0) batch = 65536;
    const auto t0 = std::chrono::high_resolution_clock::now();
    const std::vector<qec_decoder*> parts = parts_of(d);
    const int np = (int)parts.size();
    std::vector<int> rcs(np, QEC_OK);
    std::vector<std::string> errs(np);
    std::vector<double> dec(np, 0.0);
    if (np == 1) {  // one device: no host thread
        rcs[0] = monte_carlo_part(parts[0], seed, start, count, p, maxIter, stop, batch, &dec[0]);
        if (rcs[0]) errs[0] = last_error_cstr();
    } else {
        std::vector<std::thread> th;
        for (int j = 0; j < np; ++j) {
            const uint64_t lo = (uint64_t)shard_lo((long long)count, j, np), hi = (uint64_t)shard_lo((long long)count, j + 1, np);
            th.emplace_back([&, j, lo, hi] {
                rcs[j] = monte_carlo_part(parts[j], seed, start + lo, hi - lo, p, maxIter, stop, batch, &dec[j]);
                if (rcs[j]) errs[j] = last_error_cstr();
            });
        }
        for (auto& t : th) t.join();
    }
    unsigned long long cn[QEC_MC_NCOUNTERS_ALL] = {};
    for (int j = 0; j < np; ++j) {
        if (rcs[j]) return fail(rcs[j], "part " + std::to_string(j) + ": " + errs[j]);
        // monte_carlo_part left the part's counters in its page-locked copy, its stream synchronised
        for (int k = 0; k < QEC_MC_NCOUNTERS_ALL; ++k) cn[k] += parts[j]->mhost[k];
    }
    const auto t1 = std::chrono::high_resolution_clock::now();
    out->tested = count;
    out->withX = cn[QEC_MC_WITHX]; out->withZ = cn[QEC_MC_WITHZ];
    out->synX = cn[QEC_MC_SYNX]; out->synZ = cn[QEC_MC_SYNZ];
    out->logical = cn[QEC_MC_LOGICAL]; out->corrected = cn[QEC_MC_CORRECTED];
    out->convX = cn[QEC_MC_CONVX]; out->convZ = cn[QEC_MC_CONVZ];
    out->iterationsX = cn[QEC_MC_ITERX]; out->iterationsZ = cn[QEC_MC_ITERZ];
    out->decodeSeconds = *std::max_element(dec.begin(), dec.end());
    out->totalSeconds = std::chrono::duration<double>(t1 - t0).count();
    return QEC_OK;
}

int qec_sample_depolarizing_dev(qec_decoder* d, uint64_t seed, uint64_t start, size_t B, float p, uint8_t* x,
                                uint8_t* z, void* stream)
{
    if (!d || (B && (!x || !z))) return fail(QEC_ERR_ARG, "qec_sample_depolarizing_dev: bad argument");
    int rc = single_device_only(d, "qec_sample_depolarizing_dev");
    if (rc) return rc;
    QEC_DEVICE_SCOPE(d->device);
    return launch_sample_depolarizing(seed, start, (long long)B, d->code->n, p, x, z, static_cast<hipStream_t>(stream));
}

int qec_sample_independent_dev(qec_decoder* d, uint64_t seed, uint64_t start, size_t B, uint8_t* x, uint8_t* z, void* stream)
{
    if (!d || (B && (!x || !z))) return fail(QEC_ERR_ARG, "qec_sample_independent_dev: bad argument");
    int rc = single_device_only(d, "qec_sample_independent_dev");
    if (rc) return rc;
    if (!d->has_priors) return fail(QEC_ERR_ARG, "qec_sample_independent_dev: the decoder has no priors (qec_decoder_set_priors)");
    QEC_DEVICE_SCOPE(d->device);
    return launch_sample_independent(seed, start, (long long)B, d->code->n, d->dpri.data(), x, z,
                                     static_cast<hipStream_t>(stream));
}

int qec_sample_pauli_dev(qec_decoder* d, uint64_t seed, uint64_t start, size_t B, uint8_t* x, uint8_t* z, void* stream)
{
    if (!d || (B && (!x || !z))) return fail(QEC_ERR_ARG, "qec_sample_pauli_dev: bad argument");
    int rc = single_device_only(d, "qec_sample_pauli_dev");
    if (rc) return rc;
    if (!d->has_channel || d->cpu)
        return fail(QEC_ERR_ARG, "qec_sample_pauli_dev: the decoder has no Pauli channel (qec_decoder_set_pauli_channel)");
    QEC_DEVICE_SCOPE(d->device);
    return launch_sample_pauli(seed, start, (long long)B, d->code->n, d->dpth.data(), x, z, static_cast<hipStream_t>(stream));
}

int qec_sample_syndrome_dev(qec_decoder* d, uint64_t seed, uint64_t start, size_t B, float p, uint8_t* sX, uint8_t* sZ,
                            uint8_t* errp, void* stream)
{
    if (!d || (B && (!sX || !sZ))) return fail(QEC_ERR_ARG, "qec_sample_syndrome_dev: bad argument");
    int rc = single_device_only(d, "qec_sample_syndrome_dev");
    if (rc) return rc;
    QEC_DEVICE_SCOPE(d->device);
    McArgsHost h;
    h.code = d->code.get();
    h.seed = seed; h.start = start; h.p = p;
    h.sX = sX; h.sZ = sZ; h.errp = errp;
    h.chkVar = syndrome_table(d);
    h.varEdge = variable_table(d);
    h.B = (long long)B;
    h.prior = d->prior_dev();
    h.pauli_thr = d->has_channel ? d->dpth.data() : nullptr;
    rc = launch_mc_errors_syndrome(d->has_channel ? MC_SRC_PAULI : d->has_priors ? MC_SRC_INDEPENDENT : MC_SRC_PHILOX, h,
                                   static_cast<hipStream_t>(stream));
    if (rc || !d->soft_on()) return rc;
    // syndrome priors: the measurement-error channel of qec_flip_syndrome_dev, same seed and sample index
    return launch_flip_syndrome(seed, start, (long long)B, d->code->mX, d->code->mZ, d->synq_dev(), sX, sZ, nullptr, nullptr,
                                static_cast<hipStream_t>(stream));
}

int qec_syndrome_dev(qec_decoder* d, const uint8_t* x, const uint8_t* z, size_t B, uint8_t* sX, uint8_t* sZ,
                     void* stream)
{
    if (!d || (B && (!x || !z || !sX || !sZ))) return fail(QEC_ERR_ARG, "qec_syndrome_dev: bad argument");
    int rc = single_device_only(d, "qec_syndrome_dev");
    if (rc) return rc;
    QEC_DEVICE_SCOPE(d->device);
    McArgsHost h;
    h.code = d->code.get();
    h.x = x; h.z = z;
    h.sX = sX; h.sZ = sZ;
    h.chkVar = syndrome_table(d);
    h.B = (long long)B;
    return launch_mc_errors_syndrome(MC_SRC_BYTES, h, static_cast<hipStream_t>(stream));
}

int qec_pack_decisions_dev(qec_decoder* d, const uint8_t* eX, const uint8_t* eZ, const uint8_t* flags, size_t B,
                           uint8_t* out, void* stream)
{
    if (!d || (B && (!eX || !eZ || !flags || !out))) return fail(QEC_ERR_ARG, "qec_pack_decisions_dev: bad argument");
    if (B > (size_t)1 << 36) return fail(QEC_ERR_ARG, "qec_pack_decisions_dev: batch too large");
    int rc = single_device_only(d, "qec_pack_decisions_dev");
    if (rc) return rc;
    QEC_DEVICE_SCOPE(d->device);
    return launch_pack_decisions(eX, eZ, flags, (long long)B, d->code->n, out, static_cast<hipStream_t>(stream));
}

int qec_statistics_dev(qec_decoder* d, const uint8_t* x, const uint8_t* z, const uint8_t* eX, const uint8_t* eZ,
                       const uint8_t* flags, size_t B, uint64_t* counters, void* stream)
{
    if (!d || !counters || (B && (!x || !z || !eX || !eZ || !flags)))
        return fail(QEC_ERR_ARG, "qec_statistics_dev: bad argument");
    if (d->code->imp.empty()) return fail(QEC_ERR_UNSUPPORTED, "qec_statistics_dev: code has no I-P matrix");
    int rc = single_device_only(d, "qec_statistics_dev");
    if (rc) return rc;
    QEC_DEVICE_SCOPE(d->device);
    return launch_statistics(*d->code, d->imp_cols.data(), x, z, eX, eZ, flags, (long long)B,
                             reinterpret_cast<unsigned long long*>(counters), static_cast<hipStream_t>(stream));
}

int qec_statistics_packed_dev(qec_decoder* d, const uint8_t* errp, const uint8_t* records, const int32_t* iters,
                              size_t B, uint64_t* counters, void* stream)
{
    if (!d || !counters || (B && (!errp || !records))) return fail(QEC_ERR_ARG, "qec_statistics_packed_dev: bad argument");
    if (d->code->imp.empty()) return fail(QEC_ERR_UNSUPPORTED, "qec_statistics_packed_dev: code has no I-P matrix");
    int rc = single_device_only(d, "qec_statistics_packed_dev");
    if (rc) return rc;
    QEC_DEVICE_SCOPE(d->device);
    return launch_statistics_packed(*d->code, d->imp_cols.data(), errp, 2 * ((d->code->n + 7) / 8), records, iters, (long long)B,
                                    reinterpret_cast<unsigned long long*>(counters), static_cast<hipStream_t>(stream));
}

int qec_logical_packed_dev(qec_decoder* d, const uint8_t* errp, const uint8_t* records, size_t B, uint8_t* outcome,
                           void* stream)
{
    if (!d || (B && (!errp || !records || !outcome))) return fail(QEC_ERR_ARG, "qec_logical_packed_dev: bad argument");
    if (B > (size_t)1 << 36) return fail(QEC_ERR_ARG, "qec_logical_packed_dev: batch too large");
    int rc = single_device_only(d, "qec_logical_packed_dev");
    if (rc) return rc;
    if (d->code->imp.empty()) return fail(QEC_ERR_UNSUPPORTED, "qec_logical_packed_dev: code has no I-P matrix");
    QEC_DEVICE_SCOPE(d->device);
    return launch_logical_outcome(*d->code, d->imp_cols.data(), errp, records, (long long)B, outcome,
                                  static_cast<hipStream_t>(stream));
}

int qec_osd_dev(qec_decoder* d, const uint8_t* sX, const uint8_t* sZ, size_t B, const float* q, uint8_t* eX, uint8_t* eZ,
                uint8_t* flags, void* stream)
{
    if (!d || (B && (!sX || !sZ || !q || !eX || !eZ || !flags))) return fail(QEC_ERR_ARG, "qec_osd_dev: bad argument");
    int rc = single_device_only(d, "qec_osd_dev");
    if (rc) return rc;
    if (!d->odev) return fail(QEC_ERR_UNSUPPORTED, d->osd_why);
    QEC_DEVICE_SCOPE(d->device);
    // the kernel reads only the handle's tables: no workspace, no allocation, nothing to order
    return launch_osd(d->odev, d->osd_sweep, d->osd_order, sX, sZ, (long long)B, q, eX, eZ, flags, nullptr, nullptr,
                      d->osw_dev(), static_cast<hipStream_t>(stream), d->bp_method == 1);
}

int qec_osd(qec_decoder* d, const uint8_t* sX, const uint8_t* sZ, size_t B, const float* q, uint8_t* eX, uint8_t* eZ,
            uint8_t* flags)
{
    if (!d || (B && (!sX || !sZ || !q || !eX || !eZ || !flags))) return fail(QEC_ERR_ARG, "qec_osd: bad argument");
    d->osd_sectors = d->osd_cs_sectors = 0;
    for (qec_decoder* p : d->parts) p->osd_sectors = p->osd_cs_sectors = 0;
    if (B == 0) return QEC_OK;
    if (d->cpu) {
        long long swept = 0;
        d->osd_sectors = (unsigned long long)osd_host_batch(*d->oplan, sX, sZ, (long long)B, q, eX, eZ, flags, 0,
                                                            d->osd_order, &swept, d->osw_host(), d->bp_method == 1);
        d->osd_cs_sectors = (unsigned long long)swept;
        return QEC_OK;
    }
    qec_decoder* w = d->parts.empty() ? d : d->parts[0];  // a group's first part does the work
    if (!w->odev) return fail(QEC_ERR_UNSUPPORTED, w->osd_why);
    QEC_DEVICE_SCOPE(w->device);
    const Code& c = *w->code;
    const size_t qn = (size_t)(c.mX + c.mZ) * c.stride();
    hipStream_t st = w->stream;
    std::vector<uint8_t> f0(flags, flags + B);
    uint32_t swept = 0;
    try {
        DeviceArray<uint8_t> dsX(B * c.mX), dsZ(B * c.mZ), deX(B * c.n), deZ(B * c.n), dfl(B);
        DeviceArray<float> dq(B * qn);
        QEC_HIP_CHECK(hipMemcpyAsync(dsX.data(), sX, B * c.mX, hipMemcpyHostToDevice, st));
        QEC_HIP_CHECK(hipMemcpyAsync(dsZ.data(), sZ, B * c.mZ, hipMemcpyHostToDevice, st));
        QEC_HIP_CHECK(hipMemcpyAsync(deX.data(), eX, B * c.n, hipMemcpyHostToDevice, st));
        QEC_HIP_CHECK(hipMemcpyAsync(deZ.data(), eZ, B * c.n, hipMemcpyHostToDevice, st));
        QEC_HIP_CHECK(hipMemcpyAsync(dfl.data(), flags, B, hipMemcpyHostToDevice, st));
        QEC_HIP_CHECK(hipMemcpyAsync(dq.data(), q, B * qn * sizeof(float), hipMemcpyHostToDevice, st));
        QEC_HIP_CHECK(hipMemsetAsync(w->ocnt.data() + 2, 0, sizeof(uint32_t), st));
        const int rc = launch_osd(w->odev, w->osd_sweep, w->osd_order, dsX.data(), dsZ.data(), (long long)B, dq.data(),
                                  deX.data(), deZ.data(), dfl.data(), nullptr, w->ocnt.data() + 2, w->osw_dev(), st,
                                  w->bp_method == 1);
        if (rc) return rc;
        QEC_HIP_CHECK(hipMemcpyAsync(&swept, w->ocnt.data() + 2, sizeof swept, hipMemcpyDeviceToHost, st));
        QEC_HIP_CHECK(hipMemcpyAsync(eX, deX.data(), B * c.n, hipMemcpyDeviceToHost, st));
        QEC_HIP_CHECK(hipMemcpyAsync(eZ, deZ.data(), B * c.n, hipMemcpyDeviceToHost, st));
        QEC_HIP_CHECK(hipMemcpyAsync(flags, dfl.data(), B, hipMemcpyDeviceToHost, st));
        QEC_HIP_CHECK(hipStreamSynchronize(st));
    } catch (const std::exception& ex) {
        return fail(QEC_ERR_NOMEM, std::string("qec_osd: ") + ex.what());
    }
    for (size_t b = 0; b < B; ++b) w->osd_sectors += __builtin_popcount((unsigned)(f0[b] & (uint8_t)~flags[b] & QEC_SYNDROME_FAIL_XZ));
    w->osd_cs_sectors = swept;
    return QEC_OK;
}

}  // extern "C"
