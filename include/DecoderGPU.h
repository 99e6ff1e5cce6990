// DecoderGPU.h -- the reference's named GPU slot (QEC_LDPC/DecoderGPU.h:11-281),
// now backed by the MI355X engine in libqecldpc.so.  Same class name, same
// constructor and method signatures, so QEC_LDPC/main.cu's loop switches engines by
// replacing `DecoderCPU decoder(code);` with `DecoderGPU decoder(code);`.
//
// Added: DecodeBatch / DecodeBatchPacked (the batched boundary the GPU engine is built for), and
// a multi-device constructor: DecoderGPU(code, {0, 1, ..., 7}) spreads GetStatistics' samples
// (and batched decodes) over the listed GPUs with counters identical to one device
// (qec_decoder_create_multi).  Decode() keeps the reference's one-syndrome-pair semantics (a
// batch of one: one launch, copies and a synchronisation per call -- loop DecodeBatch instead).
#pragma once
#include <cstdint>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "Decoder.h"

class DecoderGPU : public Decoder {
public:
    // DecoderGPU.h:117; device = HIP ordinal
    explicit DecoderGPU(Quantum_LDPC_Code code, int device = 0) : Decoder(code)
    {
        dec_ = qec_decoder_create(_code.handle(), device, 0);
        if (!dec_) throw std::string(qec_last_error());
    }
    // an explicit engine (QEC_ENGINE_*), e.g. QEC_ENGINE_SPARSE for a circulant code that is to take priors
    DecoderGPU(Quantum_LDPC_Code code, int device, int engine) : Decoder(code)
    {
        dec_ = qec_decoder_create_engine(_code.handle(), device, 0, engine);
        if (!dec_) throw std::string(qec_last_error());
    }
    // several GPUs of this node (a device may repeat); every call shards its samples over them
    DecoderGPU(Quantum_LDPC_Code code, const std::vector<int>& devices) : Decoder(code)
    {
        dec_ = qec_decoder_create_multi(_code.handle(), devices.data(), (int)devices.size(), 0);
        if (!dec_) throw std::string(qec_last_error());
    }
    ~DecoderGPU() override { qec_decoder_destroy(dec_); }
    DecoderGPU(const DecoderGPU&) = delete;
    DecoderGPU& operator=(const DecoderGPU&) = delete;

    // Decoder::Decode (Decoder.h:40-41) with DecoderCPU::Decode semantics (DecoderCPU.h:317-390)
    ErrorCode Decode(const IntArray1d_h& syndromeX, const IntArray1d_h& syndromeZ, float errorProbability,
                     int maxIterations, IntArray1d_h& outErrorsX, IntArray1d_h& outErrorsZ) override
    {
        std::vector<uint8_t> sx = syndrome_bytes(syndromeX), sz = syndrome_bytes(syndromeZ);
        std::vector<uint8_t> ex(_code.n), ez(_code.n);
        uint8_t flags = 0;
        check(qec_decode_batch(dec_, sx.data(), sz.data(), 1, errorProbability, maxIterations, QEC_STOP_REF, ex.data(),
                               ez.data(), &flags, nullptr, nullptr));
        outErrorsX.assign(ex.begin(), ex.end());
        outErrorsZ.assign(ez.begin(), ez.end());
        return static_cast<ErrorCode>(flags);
    }

    // B syndrome pairs at once: sX [B*numEqsX], sZ [B*numEqsZ] -> eX, eZ [B*n], flags [B]
    void DecodeBatch(const std::vector<uint8_t>& sX, const std::vector<uint8_t>& sZ, size_t B, float errorProbability,
                     int maxIterations, int stopRule, std::vector<uint8_t>& eX, std::vector<uint8_t>& eZ,
                     std::vector<uint8_t>& flags)
    {
        eX.resize(B * _code.n);
        eZ.resize(B * _code.n);
        flags.resize(B);
        check(qec_decode_batch(dec_, sX.data(), sZ.data(), B, errorProbability, maxIterations, stopRule, eX.data(),
                               eZ.data(), flags.data(), nullptr, nullptr));
    }

    // B syndrome pairs -> packed decision records [B * QEC_RECORD_BYTES(n)] (eX bits, eZ bits, flags)
    void DecodeBatchPacked(const std::vector<uint8_t>& sX, const std::vector<uint8_t>& sZ, size_t B,
                           float errorProbability, int maxIterations, int stopRule, std::vector<uint8_t>& records)
    {
        records.resize(B * QEC_RECORD_BYTES(_code.n));
        check(qec_decode_batch_packed(dec_, sX.data(), sZ.data(), B, errorProbability, maxIterations, stopRule,
                                      records.data(), nullptr));
    }

    // DecoderGPU::GetStats (DecoderGPU.h:193-228): statistics over pre-generated flat
    // COUNT x n error arrays (the reference's stub decoded nothing; this one decodes).
    CodeStatistics GetStats(int errorWeight, int numErrors, float errorProbability, int maxIterations, int seed,
                            std::vector<int>& xErrors, std::vector<int>& zErrors)
    {
        const int n = _code.n;
        const size_t B = (size_t)numErrors;
        std::vector<uint8_t> x(B * n), z(B * n), sx(B * _code.numEqsX), sz(B * _code.numEqsZ);
        for (size_t k = 0; k < B * n; ++k) { x[k] = (uint8_t)(xErrors[k] & 1); z[k] = (uint8_t)(zErrors[k] & 1); }
        check(qec_code_syndrome(_code.handle(), 0, x.data(), B, sx.data()));
        check(qec_code_syndrome(_code.handle(), 1, z.data(), B, sz.data()));
        std::vector<uint8_t> ex, ez, fl;
        DecodeBatch(sx, sz, B, errorProbability, maxIterations, QEC_STOP_REF, ex, ez, fl);
        std::vector<uint8_t> rx(n), rz(n);
        CodeStatistics st{_code, (unsigned)seed, (unsigned)numErrors, 0, 0, (unsigned)errorWeight, 0, 0, 0, 0, 0, 0, 0};
        for (size_t b = 0; b < B; ++b) {
            bool ax = false, az = false;
            for (int v = 0; v < n; ++v) { ax |= x[b * n + v] != 0; az |= z[b * n + v] != 0; }
            st.numXErrorsTested += ax;
            st.numZErrorsTested += az;
            const bool dEX = fl[b] & SYNDROME_FAIL_X, dEZ = fl[b] & SYNDROME_FAIL_Z;
            st.syndromeErrorsX += dEX;
            st.syndromeErrorsZ += dEZ;
            if (!(dEX || dEZ)) {
                for (int v = 0; v < n; ++v) {
                    rx[v] = (x[b * n + v] + ex[b * n + v]) % 2;
                    rz[v] = (z[b * n + v] + ez[b * n + v]) % 2;
                }
                uint8_t le = 0;
                check(qec_code_check_logical(_code.handle(), rx.data(), rz.data(), 1, &le));
                if (le) ++st.logicalErrors; else ++st.corrected;
            }
            st.convergenceFailX += (fl[b] & CONVERGENCE_FAIL_X) != 0;
            st.convergenceFailZ += (fl[b] & CONVERGENCE_FAIL_Z) != 0;
        }
        return st;
    }

    // Decoder::GetStatistics (DecoderCPU.h:392-530 semantics; errors drawn from the same
    // mt19937(seed) stream as the reference, decoded in GPU batches)
    CodeStatistics GetStatistics(int errorWeight, int numErrors, float errorProbability, int maxIterations,
                                 unsigned int seed) override
    {
        qec_stats s{};
        check(qec_get_statistics(dec_, errorWeight, numErrors, errorProbability, maxIterations, seed, 1, &s));
        return CodeStatistics{_code, s.randSeed, s.numErrorsTested, s.numXErrorsTested, s.numZErrorsTested,
                              s.errorWeight, s.corrected, s.syndromeErrorsX, s.syndromeErrorsZ, s.logicalErrors,
                              s.convergenceFailX, s.convergenceFailZ, (long long)s.durationMicroSeconds};
    }
    CodeStatistics GetStatistics(int errorWeight, int numErrors, float errorProbability, int maxIterations) override
    {
        std::random_device rd;
        return GetStatistics(errorWeight, numErrors, errorProbability, maxIterations, rd());
    }

    std::string Describe() const
    {
        char buf[256];
        qec_decoder_describe(dec_, buf, sizeof buf);
        return buf;
    }
    // BP + OSD post-processing (QEC_OPT_OSD): order 0 is OSD-0, 1 .. 64 the combination sweep over that
    // many of the most suspicious non-pivot columns (QEC_OPT_OSD_ORDER); a negative order turns it off.
    // iterations: the soft decode that orders the columns (QEC_OPT_OSD_ITERATIONS, >= 1).
    void SetOsd(int order, int iterations = 3)
    {
        check(qec_decoder_set_option(dec_, QEC_OPT_OSD_ORDER, order > 0 ? order : 0));
        check(qec_decoder_set_option(dec_, QEC_OPT_OSD_ITERATIONS, iterations));
        check(qec_decoder_set_option(dec_, QEC_OPT_OSD, order >= 0 ? 1 : 0));
    }
    // How the combination sweep scores its candidates (QEC_OPT_OSD_SCORE): 0 by Hamming weight (the default),
    // 1 by likelihood under the priors of SetPriors (the sum of the flipped qubits' integer log-likelihood
    // weights; without priors the value has no effect).  Any other value throws the library's message.
    void SetOsdScore(int rule) { check(qec_decoder_set_option(dec_, QEC_OPT_OSD_SCORE, rule)); }
    // Per-qubit priors (qec_decoder_set_priors): priorX[v] / priorZ[v] is the prior that bit v of the X / Z
    // estimate is 1 (n entries each, 0 <= pi <= 1).  While set, BP uses them and the errorProbability argument
    // of Decode, DecodeBatch and GetStatistics is not used.  The sparse-graph engine takes them; a decoder
    // on the wave-circulant engine throws the library's message (construct it with QEC_ENGINE_SPARSE).
    void SetPriors(const std::vector<float>& priorX, const std::vector<float>& priorZ)
    {
        if (priorX.size() != (size_t)_code.n || priorZ.size() != (size_t)_code.n)
            throw std::string("SetPriors: priorX and priorZ need n entries each");
        check(qec_decoder_set_priors(dec_, priorX.data(), priorZ.data()));
    }
    void ClearPriors() { check(qec_decoder_set_priors(dec_, nullptr, nullptr)); }
    // The correlated form (QEC_OPT_CORRELATED): 0 = both sectors independently (the default), 1 = sector X first and
    // sector Z under priors conditioned on the X estimate, 2 = Z first.  Any other value throws the library's message.
    void SetCorrelated(int order) override { check(qec_decoder_set_option(dec_, QEC_OPT_CORRELATED, order)); }
    // The BP schedule (QEC_OPT_BP_SCHEDULE): 0 = flooding (the default), 1 = the serial (layered) schedule on the
    // sparse-graph engine.  Any other value, 1 on a wave-circulant decoder and 1 together with SetCorrelated(1 | 2)
    // throw the library's message.
    void SetBpSchedule(int schedule) override { check(qec_decoder_set_option(dec_, QEC_OPT_BP_SCHEDULE, schedule)); }
    // The BP message rule (QEC_OPT_BP_METHOD): 0 = the product rule (the default), 1 = scaled min-sum in the LLR domain
    // with alpha = scale / 256 (QEC_OPT_MINSUM_SCALE, 1 .. 256) on the sparse-graph engine.  Any other value, 1 together with
    // SetCorrelated(1 | 2) or SetBpSchedule(1) and 1 on a wave-circulant decoder throw the library's message.
    void SetBpMethod(int method, int scale = 160) override
    {
        check(qec_decoder_set_option(dec_, QEC_OPT_MINSUM_SCALE, scale));
        check(qec_decoder_set_option(dec_, QEC_OPT_BP_METHOD, method));
    }
    // The order of min-sum's updates (QEC_OPT_MINSUM_SCHEDULE): 0 = flooding (the default), 1 = layered (check-sequential)
    // min-sum on the sparse-graph engine.  In effect while SetBpMethod(1) is and no relay is set; independent of
    // SetBpSchedule, the product rule's serial schedule.  Any other value and 1 on a wave-circulant decoder throws the library's message.
    void SetMinSumSchedule(int schedule) { check(qec_decoder_set_option(dec_, QEC_OPT_MINSUM_SCHEDULE, schedule)); }
    // The kernels of plain min-sum decodes (QEC_OPT_MINSUM_WAVE): 0 = the sparse-graph MINSUM kernels (the default),
    // 1 = the register-resident wave kernels, bit-identical, for circulant codes with P <= 64 and a block shape of the
    // runtime-shift table (qec_code_has_wave_minsum).  A kernel choice of a sparse-engine decoder: 1 on any other
    // decoder or code throws the library's message.  In effect while SetBpMethod(1) is and no relay is set.
    void SetMinSumWave(int on) { check(qec_decoder_set_option(dec_, QEC_OPT_MINSUM_WAVE, on)); }
    // The kernels of relay decodes (QEC_OPT_RELAY_WAVE): 0 = the sparse-graph RELAY kernels (the default), 1 = the
    // register-resident wave relay kernels, bit-identical, for the codes of SetMinSumWave.  Independent of
    // SetMinSumWave; in effect while SetBpMethod(1) is and a relay is set.  1 on any other decoder or code throws the
    // library's message.
    void SetRelayWave(int on) { check(qec_decoder_set_option(dec_, QEC_OPT_RELAY_WAVE, on)); }
    // Relay-BP (qec_decoder_set_relay): `legs` legs of memory min-sum under SetBpMethod(1), gammaX / gammaZ the memory
    // strengths [legs][n] (|gamma| <= 1), stopping at the first solution or at the lightest of the first `solutions`.
    // The sparse-graph engine takes them; a wave-circulant decoder throws the library's message.
    void SetRelay(const std::vector<float>& gammaX, const std::vector<float>& gammaZ, int legs, int solutions = 1)
    {
        if (legs < 1 || gammaX.size() != (size_t)legs * _code.n || gammaZ.size() != (size_t)legs * _code.n)
            throw std::string("SetRelay: gammaX and gammaZ need legs * n entries each");
        check(qec_decoder_set_relay(dec_, gammaX.data(), gammaZ.data(), legs, solutions));
    }
    void ClearRelay() { check(qec_decoder_set_relay(dec_, nullptr, nullptr, 0, 0)); }
    // Noisy syndromes (qec_decoder_set_syndrome_priors): qX [numEqsX], qZ [numEqsZ] = the probability that each check's
    // measured bit is flipped.  Under SetBpMethod(1) every decode then treats the syndrome bits as soft; not together
    // with SetRelay or SetOsd, which throw the library's message (as this call does after them).
    void SetSyndromePriors(const std::vector<float>& qX, const std::vector<float>& qZ)
    {
        if (qX.size() != (size_t)_code.numEqsX || qZ.size() != (size_t)_code.numEqsZ)
            throw std::string("SetSyndromePriors: qX needs numEqsX and qZ numEqsZ entries");
        check(qec_decoder_set_syndrome_priors(dec_, qX.data(), qZ.data()));
    }
    void ClearSyndromePriors() { check(qec_decoder_set_syndrome_priors(dec_, nullptr, nullptr)); }
    // Per-qubit Pauli channel (qec_decoder_set_pauli_channel): qubit v suffers X, Y or Z with probabilities pX[v],
    // pY[v], pZ[v] (n entries each; Y sets both bits).  Installs the marginal priors, the conditional tables of
    // SetCorrelated and the noise of the device Monte-Carlo run; a later SetPriors or ClearPriors drops it.
    void SetPauliChannel(const std::vector<float>& pX, const std::vector<float>& pY, const std::vector<float>& pZ) override
    {
        if (pX.size() != (size_t)_code.n || pY.size() != (size_t)_code.n || pZ.size() != (size_t)_code.n)
            throw std::string("SetPauliChannel: pX, pY and pZ need n = " + std::to_string(_code.n) + " entries each");
        check(qec_decoder_set_pauli_channel(dec_, pX.data(), pY.data(), pZ.data()));
    }
    qec_decoder* handle() { return dec_; }

private:
    qec_decoder* dec_ = nullptr;
    static void check(int rc)
    {
        if (rc != QEC_OK) throw std::string(qec_last_error());
    }
};
