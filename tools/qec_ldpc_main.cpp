// qec_ldpc -- the reference's Monte-Carlo driver (QEC_LDPC/main.cu:43-118) on the
// MI355X engine.  Same init-file format ("codeFile w W COUNT MAX p", main.cu:74-88),
// same results files (results/<code>_W_<w>_MAX_<MAX>_p_<p>.txt, appended,
// main.cu:91-104) and the same output_log.txt journal (main.cu:45-52,114).
// The only change vs main.cu is the engine: DecoderGPU instead of DecoderCPU.
// Exit status is 0 on success (main.cu returns 1).
// Optional flags before the init file ("Config / flags"):
//   --engine gpu|sparse|cpu   the decoder: DecoderGPU (default; the library's choice of GPU engine), DecoderGPU on
//                      the sparse-graph engine (one GPU), or DecoderCPU (host threads, no GPU needed)
//   --gpus N           GPUs 0..N-1 of this node, one decoder spanning them (counters identical to one GPU)
//   --devices 0,3,5    the same for a list of GPUs
//   --rng msvc|philox  msvc (default): main.cu's loop, fixed-weight errors w..W from the reference's
//                      mt19937 stream (GetStatistics, reference stop rule).  philox: COUNT i.i.d.
//                      depolarising samples at p per run (qec_monte_carlo, GPU engine), w and W ignored
//   --stop ref|fixed|syndrome   stop rule of --rng philox runs (default ref)
//   --batch B          samples per device batch of --rng philox runs (default 2^20)
//   --seed S           Philox stream of --rng philox runs (default 0x51EC0DE).  --rng msvc: the mt19937
//                      seed of every GetStatistics call, for a repeatable run (without it each call
//                      draws its own from std::random_device, as main.cu does)
//   --logical file|reference|degenerate   the logical-error check: the code file's I-P matrix (default;
//                      main.cu's), or one derived from the two parity-check matrices after loading
//                      (qec_code_with_logical), so a code file with only its first three lines works.
//                      reference: what the shipped I-P matrices compute; degenerate: a residual that is
//                      a product of stabilizers counts as corrected
//   --osd 0            BP + OSD-0: samples whose syndrome BP leaves unsatisfied are repaired by ordered-statistics
//                      decoding (QEC_OPT_OSD) before they are counted; the value stays 0, the sweep's
//                      order is --osd-order
//   --osd-order L      with --osd 0: the combination sweep OSD-CS over the L most suspicious non-pivot
//                      columns (QEC_OPT_OSD_ORDER, 0 .. 64; default 0 = OSD-0)
//   --osd-iterations K iterations of the soft decode that orders OSD's columns (default 3; needs --osd)
//   --osd-score hamming|priors   with --osd 0: how the sweep scores its candidates (QEC_OPT_OSD_SCORE): by Hamming
//                      weight (default), or by likelihood under the priors of --priors FILE, which it then needs
//   --priors FILE      per-qubit priors (qec_decoder_set_priors) for whatever mode runs: FILE holds two lines of n
//                      decimal floats, sector X then sector Z.  BP then uses them and the init file's p is not
//                      used; --rng philox draws its errors independently per qubit from them.  Sparse-graph and
//                      CPU engines: on a code the default engine decodes with wave-circulant kernels the run
//                      fails with the library's message (use --engine sparse)
//   --correlated xz|zx the correlated form (QEC_OPT_CORRELATED): sector X first and sector Z under priors conditioned
//                      on the X estimate (xz), or Z first (zx).  Sparse-graph and CPU engines
//   --bp-schedule flooding|serial   the order of BP's updates (QEC_OPT_BP_SCHEDULE): flooding (default), or the serial
//                      (layered, check-sequential) schedule.  Sparse-graph and CPU engines; not with --correlated
//   --bp-method product|minsum   BP's message rule (QEC_OPT_BP_METHOD): the product rule (default), or scaled min-sum
//                      in the LLR domain.  Sparse-graph and CPU engines; not with --correlated or --bp-schedule serial
//   --minsum-scale K   min-sum's factor alpha = K / 256 (QEC_OPT_MINSUM_SCALE, 1 .. 256, default 160); needs
//                      --bp-method minsum
//   --minsum-schedule flooding|serial   the order of min-sum's updates (QEC_OPT_MINSUM_SCHEDULE): flooding (default), or
//                      layered (check-sequential) min-sum.  Sparse-graph and CPU engines; needs --bp-method minsum
//   --minsum-wave 0|1  the kernels of plain min-sum decodes (QEC_OPT_MINSUM_WAVE): 1 = the register-resident wave
//                      kernels (circulant codes, P <= 64, a block shape of the runtime-shift table); needs
//                      --engine sparse and --bp-method minsum
//   --relay FILE       Relay-BP (qec_decoder_set_relay): FILE holds 2 L lines of n decimal floats, the memory strengths
//                      of the L legs of sector X, then of the L legs of sector Z (each |gamma| <= 1); needs
//                      --bp-method minsum
//   --relay-solutions S   the relay stops at the lightest of its first S solutions (1 .. 64, default 1); needs --relay
//   --relay-wave 0|1   the kernels of relay decodes (QEC_OPT_RELAY_WAVE): 1 = the register-resident wave relay kernels
//                      (the codes of --minsum-wave); needs --engine sparse, --bp-method minsum and --relay FILE
//   --syndrome-priors FILE   noisy syndromes (qec_decoder_set_syndrome_priors): FILE holds two lines of decimal floats, the
//                      numEqsX flip probabilities of the X checks' measured bits, then the numEqsZ of the Z checks';
//                      needs --bp-method minsum; not with --relay or --osd.  --rng philox then flips the sampled
//                      syndromes with these probabilities
//   --syndrome-noise Q   the same with one value Q in [0, 1] for every check; not together with --syndrome-priors
//   --pauli FILE       per-qubit Pauli channel (qec_decoder_set_pauli_channel): FILE holds three lines of n decimal
//                      floats, pX, pY and pZ.  BP decodes under its marginals (and --correlated under its conditional
//                      tables), the init file's p is not used, and --rng philox draws its errors from the channel.
//                      Not together with --priors
// Unknown or inconsistent flags exit with status 2.
#include <algorithm>
#include <chrono>
#include <ctime>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "DecoderCPU.h"
#include "DecoderGPU.h"
#include "Quantum_LDPC_Code.h"

namespace {

// One --rng philox run's block in the results file (the CodeStatistics fields that exist for
// depolarising samples, plus the stop rule and the iterations executed)
void write_mc_block(std::ostream& out, const Quantum_LDPC_Code& code, unsigned long long seed, float p, int maxIter,
                    const char* stop, const qec_mc_result& r)
{
    out << "Code: " << code << std::endl
        << "Philox Seed: " << seed << std::endl
        << "Duration(micro-s): " << (long long)(r.totalSeconds * 1e6) << std::endl
        << "Physical Error Rate: " << p << std::endl
        << "Stop Rule: " << stop << std::endl
        << "Max Iterations: " << maxIter << std::endl
        << "Errors Tested: " << r.tested << std::endl
        << "Errors With X: " << r.withX << std::endl
        << "Errors With Z: " << r.withZ << std::endl
        << "Corrected: " << r.corrected << std::endl
        << "Syndrome Errors X: " << r.synX << std::endl
        << "Syndrome Errors Z: " << r.synZ << std::endl
        << "Logical Errors: " << r.logical << std::endl
        << "Convergence Fail X: " << r.convX << std::endl
        << "Convergence Fail Z: " << r.convZ << std::endl
        << "Iterations X: " << r.iterationsX << std::endl
        << "Iterations Z: " << r.iterationsZ << std::endl;
}

int usage(const std::string& why)
{
    std::cerr << why << std::endl
              << "usage: qec_ldpc [--engine gpu|sparse|cpu] [--gpus N | --devices i,j,...] [--rng msvc|philox]"
                 " [--stop ref|fixed|syndrome] [--batch B] [--seed S] [--logical file|reference|degenerate]"
                 " [--osd 0 [--osd-order L] [--osd-iterations K] [--osd-score hamming|priors]] [--priors FILE]"
                 " [--correlated xz|zx] [--bp-schedule flooding|serial] [--bp-method product|minsum [--minsum-scale K] [--minsum-wave 0|1]"
                 " [--relay FILE [--relay-solutions S] [--relay-wave 0|1]]"
                 " [--syndrome-priors FILE | --syndrome-noise Q]] [--pauli FILE] initFile"
              << std::endl;
    return 2;
}

// --priors FILE: two lines of n decimal floats (sector X, then sector Z)
void read_priors(const std::string& path, int n, std::vector<float>& pX, std::vector<float>& pZ)
{
    std::ifstream in(path);
    if (!in.is_open()) throw std::string("--priors: unable to open " + path);
    std::string line;
    for (std::vector<float>* out : {&pX, &pZ}) {
        if (!std::getline(in, line)) throw std::string("--priors: " + path + " needs two lines of n floats (X, then Z)");
        std::stringstream ss(line);
        float v;
        while (ss >> v) out->push_back(v);
        if (!ss.eof() || (int)out->size() != n)
            throw std::string("--priors: each line of " + path + " needs n = " + std::to_string(n) + " decimal floats");
    }
}

// --syndrome-priors FILE: two lines of decimal floats (mX for the X checks, then mZ for the Z checks)
void read_syndrome_priors(const std::string& path, int mX, int mZ, std::vector<float>& qX, std::vector<float>& qZ)
{
    std::ifstream in(path);
    if (!in.is_open()) throw std::string("--syndrome-priors: unable to open " + path);
    std::string line;
    for (int sec = 0; sec < 2; ++sec) {
        std::vector<float>& out = sec ? qZ : qX;
        const int m = sec ? mZ : mX;
        if (!std::getline(in, line))
            throw std::string("--syndrome-priors: " + path + " needs two lines of floats (the X checks, then the Z checks)");
        std::stringstream ss(line);
        float v;
        while (ss >> v) out.push_back(v);
        if (!ss.eof() || (int)out.size() != m)
            throw std::string("--syndrome-priors: line " + std::to_string(sec + 1) + " of " + path + " needs " +
                              std::to_string(m) + " decimal floats");
    }
}

// --pauli FILE: three lines of n decimal floats (pX, pY, pZ)
void read_pauli(const std::string& path, int n, std::vector<float> (&out)[3])
{
    std::ifstream in(path);
    if (!in.is_open()) throw std::string("--pauli: unable to open " + path);
    std::string line;
    for (std::vector<float>& o : out) {
        if (!std::getline(in, line)) throw std::string("--pauli: " + path + " needs three lines of n floats (pX, pY, pZ)");
        std::stringstream ss(line);
        float v;
        while (ss >> v) o.push_back(v);
        if (!ss.eof() || (int)o.size() != n)
            throw std::string("--pauli: each line of " + path + " needs n = " + std::to_string(n) + " decimal floats");
    }
}

// --relay FILE: 2 L lines of n decimal floats (the L legs of sector X, then the L legs of sector Z); returns L
int read_relay(const std::string& path, int n, std::vector<float>& gX, std::vector<float>& gZ)
{
    std::ifstream in(path);
    if (!in.is_open()) throw std::string("--relay: unable to open " + path);
    std::vector<float> all;
    std::string line;
    int lines = 0;
    while (std::getline(in, line)) {
        if (line.find_first_not_of(" \t\r") == std::string::npos) continue;
        std::stringstream ss(line);
        float v;
        int k = 0;
        while (ss >> v) { all.push_back(v); ++k; }
        if (!ss.eof() || k != n)
            throw std::string("--relay: each line of " + path + " needs n = " + std::to_string(n) + " decimal floats");
        ++lines;
    }
    if (lines == 0 || lines % 2)
        throw std::string("--relay: " + path + " needs 2 L lines of n floats (the L legs of X, then the L legs of Z)");
    const size_t half = all.size() / 2;
    gX.assign(all.begin(), all.begin() + half);
    gZ.assign(all.begin() + half, all.end());
    return lines / 2;
}

}  // namespace

int main(int argc, char** argv)
{
    std::ofstream log("output_log.txt", std::ios::app);
    if (!log.is_open()) {
        std::cerr << "Unable to open output log file" << std::endl;
        return 2;
    }
    std::time_t ts = std::chrono::system_clock::to_time_t(std::chrono::system_clock::now());
    log << std::endl << std::ctime(&ts);
    std::vector<int> devices{0};
    std::string engine = "gpu", rng = "msvc", stopName = "ref", logical = "file", priorsFile, pauliFile, relayFile;
    std::string synPriorsFile;
    float synNoise = 0.0f;
    bool synNoiseFlag = false;
    int relaySolutions = 1;
    bool relaySolutionsFlag = false;
    int correlated = 0, bpSchedule = 0, bpMethod = 0, minsumScale = 160;
    bool minsumScaleFlag = false;
    int minsumWave = 0, relayWave = 0, minsumSchedule = 0;
    bool minsumScheduleFlag = false;
    bool relayWaveFlag = false;
    bool deviceFlag = false, stopFlag = false, batchFlag = false, seedFlag = false, osd = false, osdIterFlag = false;
    bool osdOrderFlag = false, osdScoreFlag = false;
    int osdScore = 0;
    int osdIterations = 3, osdOrder = 0;
    size_t batch = size_t(1) << 20;
    unsigned long long seed = 0x51EC0DE;
    int a = 1;
    try {
        for (; a + 1 < argc && std::string(argv[a]).rfind("--", 0) == 0; a += 2) {
            const std::string flag = argv[a], val = argv[a + 1];
            if (flag == "--gpus" || flag == "--devices") {
                devices.clear();
                deviceFlag = true;
                if (flag == "--gpus") {
                    for (int k = 0; k < std::stoi(val); ++k) devices.push_back(k);
                } else {
                    std::stringstream ss(val);
                    std::string tok;
                    while (std::getline(ss, tok, ',')) devices.push_back(std::stoi(tok));
                }
            } else if (flag == "--engine") {
                engine = val;
                if (engine != "gpu" && engine != "sparse" && engine != "cpu") return usage("--engine: gpu, sparse or cpu");
            } else if (flag == "--rng") {
                rng = val;
                if (rng != "msvc" && rng != "philox") return usage("--rng: msvc or philox");
            } else if (flag == "--stop") {
                stopName = val;
                stopFlag = true;
                if (stopName != "ref" && stopName != "fixed" && stopName != "syndrome")
                    return usage("--stop: ref, fixed or syndrome");
            } else if (flag == "--logical") {
                logical = val;
                if (logical != "file" && logical != "reference" && logical != "degenerate")
                    return usage("--logical: file, reference or degenerate");
            } else if (flag == "--batch") {
                const long long b = std::stoll(val);
                if (b <= 0) return usage("--batch: a positive sample count");
                batch = (size_t)b;
                batchFlag = true;
            } else if (flag == "--osd") {
                if (val != "0") return usage("--osd: 0 turns the OSD stage on (its order is --osd-order)");
                osd = true;
            } else if (flag == "--osd-order") {
                size_t used = 0;
                osdOrder = std::stoi(val, &used);
                osdOrderFlag = true;
                if (used != val.size() || osdOrder < 0 || osdOrder > 64) return usage("--osd-order: 0 .. 64");
            } else if (flag == "--osd-iterations") {
                osdIterations = std::stoi(val);
                osdIterFlag = true;
                if (osdIterations < 1) return usage("--osd-iterations: at least 1");
            } else if (flag == "--osd-score") {
                if (val != "hamming" && val != "priors") return usage("--osd-score: hamming or priors");
                osdScore = val == "priors" ? 1 : 0;
                osdScoreFlag = true;
            } else if (flag == "--priors") {
                priorsFile = val;
            } else if (flag == "--pauli") {
                pauliFile = val;
            } else if (flag == "--correlated") {
                if (val != "xz" && val != "zx") return usage("--correlated: xz or zx");
                correlated = val == "xz" ? 1 : 2;
            } else if (flag == "--bp-schedule") {
                if (val != "flooding" && val != "serial") return usage("--bp-schedule: flooding or serial");
                bpSchedule = val == "serial" ? 1 : 0;
            } else if (flag == "--bp-method") {
                if (val != "product" && val != "minsum") return usage("--bp-method: product or minsum");
                bpMethod = val == "minsum" ? 1 : 0;
            } else if (flag == "--minsum-scale") {
                minsumScale = std::stoi(val);
                if (minsumScale < 1 || minsumScale > 256) return usage("--minsum-scale: 1 .. 256");
                minsumScaleFlag = true;
            } else if (flag == "--minsum-schedule") {
                if (val != "flooding" && val != "serial") return usage("--minsum-schedule: flooding or serial");
                minsumSchedule = val == "serial" ? 1 : 0;
                minsumScheduleFlag = true;
            } else if (flag == "--minsum-wave") {
                if (val != "0" && val != "1") return usage("--minsum-wave: 0 or 1");
                minsumWave = val == "1" ? 1 : 0;
            } else if (flag == "--relay-wave") {
                if (val != "0" && val != "1") return usage("--relay-wave: 0 or 1");
                relayWave = val == "1" ? 1 : 0;
                relayWaveFlag = true;
            } else if (flag == "--syndrome-priors") {
                synPriorsFile = val;
            } else if (flag == "--syndrome-noise") {
                size_t used = 0;
                synNoise = std::stof(val, &used);
                synNoiseFlag = true;
                if (used != val.size() || !(synNoise >= 0.0f && synNoise <= 1.0f)) return usage("--syndrome-noise: a value in [0, 1]");
            } else if (flag == "--relay") {
                relayFile = val;
            } else if (flag == "--relay-solutions") {
                size_t used = 0;
                relaySolutions = std::stoi(val, &used);
                relaySolutionsFlag = true;
                if (used != val.size() || relaySolutions < 1 || relaySolutions > 64) return usage("--relay-solutions: 1 .. 64");
            } else if (flag == "--seed") {
                seed = std::stoull(val, nullptr, 0);
                seedFlag = true;
            } else {
                return usage("unknown flag " + flag);
            }
        }
    } catch (const std::exception&) {
        return usage("unreadable flag value");
    }
    if (engine != "gpu" && deviceFlag) return usage("--gpus / --devices need --engine gpu");
    if (rng == "philox" && engine == "cpu") return usage("--rng philox runs on the GPU engine only");
    if (rng == "msvc" && (stopFlag || batchFlag))
        return usage("--stop / --batch apply to --rng philox (GetStatistics keeps the reference stop rule)");
    if (osdIterFlag && !osd) return usage("--osd-iterations needs --osd 0");
    if (osdOrderFlag && !osd) return usage("--osd-order needs --osd 0");
    if (osdScoreFlag && !osd) return usage("--osd-score needs --osd 0");
    if (bpSchedule && correlated) return usage("--bp-schedule serial and --correlated exclude each other");
    if (minsumScaleFlag && !bpMethod) return usage("--minsum-scale needs --bp-method minsum");
    if (minsumScheduleFlag && !bpMethod) return usage("--minsum-schedule needs --bp-method minsum");
    if (minsumWave && (!bpMethod || engine != "sparse")) return usage("--minsum-wave 1 needs --engine sparse and --bp-method minsum");
    if (bpMethod && correlated) return usage("--bp-method minsum and --correlated exclude each other");
    if (bpMethod && bpSchedule) return usage("--bp-method minsum and --bp-schedule serial exclude each other");
    if (!relayFile.empty() && !bpMethod) return usage("--relay needs --bp-method minsum");
    if (relaySolutionsFlag && relayFile.empty()) return usage("--relay-solutions needs --relay FILE");
    if (relayWaveFlag && (!bpMethod || engine != "sparse" || relayFile.empty()))
        return usage("--relay-wave needs --engine sparse, --bp-method minsum and --relay FILE");
    const bool soft = synNoiseFlag || !synPriorsFile.empty();
    if (synNoiseFlag && !synPriorsFile.empty()) return usage("--syndrome-noise and --syndrome-priors exclude each other");
    if (soft && !bpMethod) return usage("--syndrome-priors / --syndrome-noise need --bp-method minsum");
    if (soft && !relayFile.empty()) return usage("--syndrome-priors / --syndrome-noise and --relay exclude each other");
    if (soft && osd) return usage("--syndrome-priors / --syndrome-noise and --osd exclude each other");
    if (!pauliFile.empty() && !priorsFile.empty()) return usage("--pauli and --priors exclude each other");
    if (osdScore == 1 && priorsFile.empty()) return usage("--osd-score priors needs --priors FILE");
    if (argc - a != 1 || devices.empty()) {
        log << "Must provide initialization file." << std::endl;
        return 0;
    }
    std::string initFile = argv[a];
    std::ifstream init(initFile);
    if (!init.is_open()) {
        log << "Unable to open init file \"" << initFile
            << "\". Please make sure the file exists in the current directory." << std::endl;
        return 0;
    }
    log << "Initializing run from file " << initFile << std::endl;
    std::string codeFile;
    init >> codeFile;
    try {
        std::cout << "Creating code from file " << codeFile << std::endl;
        Quantum_LDPC_Code code = Quantum_LDPC_Code::createFromFile(codeFile);
        if (logical != "file")
            code = code.withLogicalCheck(logical == "reference" ? QEC_LOGICAL_REFERENCE : QEC_LOGICAL_DEGENERATE);
        int w, W, COUNT, MAX_ITERATIONS;
        float p;
        init >> w >> W >> COUNT >> MAX_ITERATIONS >> p;
        const bool read_ok = !init.fail();
        init.close();
        if (!read_ok || COUNT < 0 || MAX_ITERATIONS < 0) {
            // main.cu:74-88 reads the same fields; a negative or unread COUNT would wrap to ~1.8e19 samples
            // in the Philox run below (main.cu's own loop just does nothing then)
            std::cerr << initFile << ": expected 'codeFile w W COUNT MAX p' with COUNT >= 0 and MAX >= 0" << std::endl;
            return 2;
        }
        std::vector<float> priorX, priorZ;
        if (!priorsFile.empty()) read_priors(priorsFile, code.n, priorX, priorZ);
        std::vector<float> pauli[3];
        if (!pauliFile.empty()) read_pauli(pauliFile, code.n, pauli);
        std::vector<float> gammaX, gammaZ;
        const int relayLegs = relayFile.empty() ? 0 : read_relay(relayFile, code.n, gammaX, gammaZ);
        std::vector<float> synX, synZ;
        if (!synPriorsFile.empty()) read_syndrome_priors(synPriorsFile, code.numEqsX, code.numEqsZ, synX, synZ);
        if (synNoiseFlag) { synX.assign(code.numEqsX, synNoise); synZ.assign(code.numEqsZ, synNoise); }
        if (rng == "philox") {
            std::unique_ptr<DecoderGPU> dp(engine == "sparse" ? new DecoderGPU(code, 0, QEC_ENGINE_SPARSE)
                                                               : new DecoderGPU(code, devices));
            DecoderGPU& decoder = *dp;
            if (osd) decoder.SetOsd(osdOrder, osdIterations);
            if (osd) decoder.SetOsdScore(osdScore);
            if (!priorsFile.empty()) decoder.SetPriors(priorX, priorZ);
            if (!pauliFile.empty()) decoder.SetPauliChannel(pauli[0], pauli[1], pauli[2]);
            if (correlated) decoder.SetCorrelated(correlated);
            if (bpSchedule) decoder.SetBpSchedule(bpSchedule);
            if (bpMethod) decoder.SetBpMethod(bpMethod, minsumScale);
            if (minsumSchedule) decoder.SetMinSumSchedule(minsumSchedule);
            if (minsumWave) decoder.SetMinSumWave(minsumWave);
            if (relayLegs) decoder.SetRelay(gammaX, gammaZ, relayLegs, relaySolutions);
            if (relayWave) decoder.SetRelayWave(relayWave);
            if (soft) decoder.SetSyndromePriors(synX, synZ);
            std::cout << "Engine: " << decoder.Describe() << std::endl;
            const int stop = stopName == "ref" ? QEC_STOP_REF : stopName == "fixed" ? QEC_STOP_FIXED : QEC_STOP_SYNDROME;
            std::stringstream fileName;
            fileName << "results/" << code << "_DEPOLARIZING_MAX_" << MAX_ITERATIONS << "_p_" << p << "_" << stopName
                     << ".txt";
            std::string str = fileName.str();
            str.erase(std::remove(str.begin(), str.end(), ' '), str.end());
            std::cout << str << std::endl;
            std::ofstream outFile(str, std::ios_base::app);
            qec_mc_result r{};
            if (qec_monte_carlo(decoder.handle(), seed, 0, (uint64_t)COUNT, p, MAX_ITERATIONS, stop, batch, &r) != QEC_OK)
                throw std::string(qec_last_error());
            write_mc_block(outFile, code, seed, p, MAX_ITERATIONS, stopName.c_str(), r);
            outFile << std::endl;
            log << "Run complete." << std::endl;
            return 0;
        }
        std::unique_ptr<Decoder> decoder;
        if (engine == "cpu") {
            DecoderCPU* c = new DecoderCPU(code);
            decoder.reset(c);
            if (osd) c->SetOsd(osdOrder, osdIterations);
            if (osd) c->SetOsdScore(osdScore);
            if (!priorsFile.empty()) c->SetPriors(priorX, priorZ);
            if (!pauliFile.empty()) c->SetPauliChannel(pauli[0], pauli[1], pauli[2]);
            if (correlated) c->SetCorrelated(correlated);
            if (bpSchedule) c->SetBpSchedule(bpSchedule);
            if (bpMethod) c->SetBpMethod(bpMethod, minsumScale);
            if (minsumSchedule) c->SetMinSumSchedule(minsumSchedule);
            if (relayLegs) c->SetRelay(gammaX, gammaZ, relayLegs, relaySolutions);
            if (soft) c->SetSyndromePriors(synX, synZ);
            std::cout << "Engine: CPU (" << std::thread::hardware_concurrency() << " threads)" << std::endl;
        } else {
            DecoderGPU* g = engine == "sparse" ? new DecoderGPU(code, 0, QEC_ENGINE_SPARSE) : new DecoderGPU(code, devices);
            decoder.reset(g);
            if (osd) g->SetOsd(osdOrder, osdIterations);
            if (osd) g->SetOsdScore(osdScore);
            if (!priorsFile.empty()) g->SetPriors(priorX, priorZ);
            if (!pauliFile.empty()) g->SetPauliChannel(pauli[0], pauli[1], pauli[2]);
            if (correlated) g->SetCorrelated(correlated);
            if (bpSchedule) g->SetBpSchedule(bpSchedule);
            if (bpMethod) g->SetBpMethod(bpMethod, minsumScale);
            if (minsumSchedule) g->SetMinSumSchedule(minsumSchedule);
            if (minsumWave) g->SetMinSumWave(minsumWave);
            if (relayLegs) g->SetRelay(gammaX, gammaZ, relayLegs, relaySolutions);
            if (relayWave) g->SetRelayWave(relayWave);
            if (soft) g->SetSyndromePriors(synX, synZ);
            std::cout << "Engine: " << g->Describe() << std::endl;
        }
        for (; w <= W; ++w) {
            std::stringstream fileName;
            fileName << "results/" << code << "_W_" << w << "_MAX_" << MAX_ITERATIONS << "_p_" << p << ".txt";
            std::string str = fileName.str();
            str.erase(std::remove(str.begin(), str.end(), ' '), str.end());
            std::cout << str << std::endl;
            std::ofstream outFile(str, std::ios_base::app);
            CodeStatistics stats = seedFlag ? decoder->GetStatistics(w, COUNT, p, MAX_ITERATIONS, (unsigned int)seed)
                                            : decoder->GetStatistics(w, COUNT, p, MAX_ITERATIONS);
            outFile << stats << std::endl << std::endl;
        }
    } catch (const std::string& s) {
        log << s << std::endl;
        std::cerr << s << std::endl;
        return 1;
    }
    log << "Run complete." << std::endl;
    return 0;
}
