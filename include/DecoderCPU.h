// DecoderCPU.h -- the reference's CPU decoder class (QEC_LDPC/DecoderCPU.h:16-530), backed by the
// CPU engine of libqecldpc.so (qec_decoder_create with device -1): host threads over edge-major
// tables, the reference's arithmetic operation for operation, so decisions, flags and
// CodeStatistics counters are bit-identical.  Same class name and signatures, so the unmodified
// `DecoderCPU decoder(code);` of QEC_LDPC/main.cu:79 builds against this repository.
//
// Decode takes the base class's std::vector arguments, so it overrides Decoder::Decode (the
// reference's cusp vectors hid it instead).
#pragma once
#include <cstdint>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "Decoder.h"

class DecoderCPU : public Decoder {
public:
    explicit DecoderCPU(Quantum_LDPC_Code code) : Decoder(code)
    {
        dec_ = qec_decoder_create(_code.handle(), -1, 0);
        if (!dec_) throw std::string(qec_last_error());
    }
    ~DecoderCPU() override { qec_decoder_destroy(dec_); }
    DecoderCPU(const DecoderCPU&) = delete;
    DecoderCPU& operator=(const DecoderCPU&) = delete;

    // DecoderCPU::Decode (DecoderCPU.h:317-390)
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

    // DecoderCPU::GetStatistics (DecoderCPU.h:392-530): tests (numErrors / nThreads) * nThreads
    // samples, nThreads = the host's hardware threads (the reference's omp_get_max_threads()).
    CodeStatistics GetStatistics(int errorWeight, int numErrors, float errorProbability, int maxIterations,
                                 unsigned int seed) override
    {
        const unsigned hw = std::thread::hardware_concurrency();
        qec_stats s{};
        check(qec_get_statistics(dec_, errorWeight, numErrors, errorProbability, maxIterations, seed, hw ? (int)hw : 1,
                                 &s));
        return CodeStatistics{_code, s.randSeed, s.numErrorsTested, s.numXErrorsTested, s.numZErrorsTested,
                              s.errorWeight, s.corrected, s.syndromeErrorsX, s.syndromeErrorsZ, s.logicalErrors,
                              s.convergenceFailX, s.convergenceFailZ, (long long)s.durationMicroSeconds};
    }
    CodeStatistics GetStatistics(int errorWeight, int numErrors, float errorProbability, int maxIterations) override
    {
        std::random_device rd;
        return GetStatistics(errorWeight, numErrors, errorProbability, maxIterations, rd());
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
    // of Decode, DecodeBatch and GetStatistics is not used.
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
    // The BP schedule (QEC_OPT_BP_SCHEDULE): 0 = flooding (the default), 1 = the serial (layered) schedule.  Any other
    // value, and 1 together with SetCorrelated(1 | 2), throws the library's message.
    void SetBpSchedule(int schedule) override { check(qec_decoder_set_option(dec_, QEC_OPT_BP_SCHEDULE, schedule)); }
    // The BP message rule (QEC_OPT_BP_METHOD): 0 = the product rule (the default), 1 = scaled min-sum in the LLR domain
    // with alpha = scale / 256 (QEC_OPT_MINSUM_SCALE, 1 .. 256).  Any other value, 1 together with
    // SetCorrelated(1 | 2) or SetBpSchedule(1) throws the library's message.
    void SetBpMethod(int method, int scale = 160) override
    {
        check(qec_decoder_set_option(dec_, QEC_OPT_MINSUM_SCALE, scale));
        check(qec_decoder_set_option(dec_, QEC_OPT_BP_METHOD, method));
    }
    // The order of min-sum's updates (QEC_OPT_MINSUM_SCHEDULE): 0 = flooding (the default), 1 = layered (check-sequential)
    // min-sum.  In effect while SetBpMethod(1) is and no relay is set; independent of
    // SetBpSchedule, the product rule's serial schedule.  Any other value throws the library's message.
    void SetMinSumSchedule(int schedule) { check(qec_decoder_set_option(dec_, QEC_OPT_MINSUM_SCHEDULE, schedule)); }
    // Relay-BP (qec_decoder_set_relay): `legs` legs of memory min-sum under SetBpMethod(1), gammaX / gammaZ the memory
    // strengths [legs][n] (|gamma| <= 1), stopping at the first solution or at the lightest of the first `solutions`.
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
