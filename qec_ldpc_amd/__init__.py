"""qec_ldpc_amd -- Python view of libqecldpc.so, the MI355X belief-propagation
decoder for quasi-cyclic CSS quantum LDPC codes.

Mirrors the reference's interface (cantwellc/QEC_LDPC):
  * Quantum_LDPC_Code.createFromFile / GetSyndromeX / GetSyndromeZ / CheckLogicalError
    (QEC_LDPC/Quantum_LDPC_Code.h:26-142)
  * QC_LDPC_CSS(J, K, L, P, sigma, tau) generator (QEC_LDPC/QEC_LDPC_CSS.cu:5-131)
  * DecoderGPU(code).Decode / GetStatistics (QEC_LDPC/Decoder.h:40-47, DecoderGPU.h:117-280)
plus the batched entry points the GPU engine is built around (decode_batch,
decode_batch_dev).  Every call goes through the C ABI declared in
include/qec_ldpc.h; there is no CPU decoding path in this package.  If the
shared object is missing the import of the library fails loudly.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libqecldpc.so")

SUCCESS = 0
SYNDROME_FAIL_X = 1
SYNDROME_FAIL_Z = 2
CONVERGENCE_FAIL_X = 4
CONVERGENCE_FAIL_Z = 8
STOP = {"ref": 0, "fixed": 1, "syndrome": 2}
ENGINE = {"auto": 0, "circulant": 1, "sparse": 2, "cpu": 3}
OPTION = {"hard_paths": 1, "cycle_jump": 2, "schedule": 3, "sector_split": 4, "phase_stats": 5, "triage": 6,
          "last_path": 7, "mc_decode_time": 8, "osd": 9, "osd_iterations": 10, "osd_sectors": 11,
          "osd_sweep": 12, "osd_order": 13, "osd_cs_sectors": 14, "near_hard": 15, "osd_score": 16,
          "correlated": 17, "bp_schedule": 18, "bp_method": 19, "minsum_scale": 20,
          "minsum_wave": 21, "relay_wave": 22, "minsum_schedule": 23, "light_memo": 24,
          "near_probe": 25}
OPTIONS = OPTION
# values of the "bp_schedule" option (QEC_OPT_BP_SCHEDULE)
BP_SCHEDULE = {"flooding": 0, "serial": 1}
# values of the "bp_method" option (QEC_OPT_BP_METHOD)
BP_METHOD = {"product": 0, "minsum": 1}
# values of the "minsum_schedule" option (QEC_OPT_MINSUM_SCHEDULE)
MINSUM_SCHEDULE = {"flooding": 0, "layered": 1}
# QEC_PATH_* bits of QEC_OPT_LAST_PATH (include/qec_ldpc.h): the launch sequence of the last decode call
PATH = {"ordered": 1, "sector_order": 2, "split_waves": 4, "sector_launches": 8, "triage": 16, "bit_rows": 32,
        "sparse": 64, "records": 128, "osd": 256, "correlated": 512, "serial": 1024,
        "minsum": 2048, "relay": 4096, "wave": 8192, "soft": 16384}

# every symbol include/qec_ldpc.h declares
EXPORTS = (
    "qec_last_error", "qec_abi_version", "qec_build_id",
    "qec_code_load", "qec_code_generate", "qec_code_from_matrices", "qec_code_degrees", "qec_code_layers",
    "qec_code_has_wave_minsum",
    "qec_code_free",
    "qec_code_params", "qec_code_exponents",
    "qec_code_pcm", "qec_code_describe", "qec_code_syndrome", "qec_code_check_logical",
    "qec_code_with_logical", "qec_code_logical_mode", "qec_code_logical_rows", "qec_code_imp",
    "qec_decoder_create", "qec_decoder_create_engine", "qec_decoder_create_multi", "qec_decoder_create_multi_engine",
    "qec_decoder_destroy",
    "qec_decoder_num_parts", "qec_decoder_part", "qec_decoder_device", "qec_decoder_describe",
    "qec_decoder_set_option", "qec_decoder_get_option", "qec_near_hard_threshold", "qec_near_probe",
    "qec_decoder_set_priors", "qec_decoder_get_priors", "qec_decoder_get_osd_weights", "qec_sample_independent_dev",
    "qec_correlated_priors", "qec_minsum_llr", "qec_decoder_get_minsum_llr", "qec_decoder_set_pauli_channel", "qec_decoder_get_pauli_channel",
    "qec_decoder_set_relay", "qec_decoder_get_relay",
    "qec_decoder_set_syndrome_priors", "qec_decoder_get_syndrome_priors",
    "qec_decode_batch_soft", "qec_decode_batch_soft_dev", "qec_flip_syndrome_dev",
    "qec_decoder_get_conditional_priors", "qec_sample_pauli_dev",
    "qec_decode_batch", "qec_decode_batch_dev", "qec_decode_batch_packed", "qec_decode_batch_packed_dev",
    "qec_decode_bits_packed_dev",
    "qec_sample_fixed_weight", "qec_get_statistics",
    "qec_sample_depolarizing_dev", "qec_sample_syndrome_dev", "qec_syndrome_dev", "qec_statistics_dev",
    "qec_statistics_packed_dev", "qec_logical_packed_dev", "qec_pack_decisions_dev",
    "qec_monte_carlo",
    "qec_osd", "qec_osd_dev",
)
# QEC_LOGICAL_*: where a code's logical check comes from (include/qec_ldpc.h)
LOGICAL = {"file": 0, "reference": 1, "degenerate": 2}
# QEC_OUTCOME_*: logical_packed_dev's per-sample outcomes
OUTCOME_CORRECTED, OUTCOME_LOGICAL, OUTCOME_SYNDROME_FAIL = 0, 1, 2
MC_COUNTERS = ("withX", "withZ", "synX", "synZ", "logical", "corrected", "convX", "convZ")
MC_COUNTERS_ALL = MC_COUNTERS + ("iterationsX", "iterationsZ")


def record_bytes(n):
    """Bytes of one packed decision record (QEC_RECORD_BYTES): eX bits, eZ bits, flags byte."""
    return 2 * ((n + 7) // 8) + 1


class QecError(RuntimeError):
    pass


class Stats(ctypes.Structure):
    """qec_stats == CodeStatistics counters (QEC_LDPC/CodeStatistics.h:5-20)."""
    _fields_ = [("randSeed", ctypes.c_uint32), ("numErrorsTested", ctypes.c_uint32),
                ("numXErrorsTested", ctypes.c_uint32), ("numZErrorsTested", ctypes.c_uint32),
                ("errorWeight", ctypes.c_uint32), ("corrected", ctypes.c_uint32),
                ("syndromeErrorsX", ctypes.c_uint32), ("syndromeErrorsZ", ctypes.c_uint32),
                ("logicalErrors", ctypes.c_uint32), ("convergenceFailX", ctypes.c_uint32),
                ("convergenceFailZ", ctypes.c_uint32), ("durationMicroSeconds", ctypes.c_int64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class MCResult(ctypes.Structure):
    """qec_mc_result: a device Monte-Carlo run's counters and timings."""
    _fields_ = [(k, ctypes.c_uint64) for k in ("tested", "withX", "withZ", "synX", "synZ", "logical", "corrected",
                                               "convX", "convZ", "iterationsX", "iterationsZ")] + \
               [("decodeSeconds", ctypes.c_double), ("totalSeconds", ctypes.c_double)]

    def as_dict(self):
        return {k: (float(getattr(self, k)) if t is ctypes.c_double else int(getattr(self, k)))
                for k, t in self._fields_}


_lib = None


def lib():
    """The loaded libqecldpc.so (raises if it was not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise QecError("libqecldpc.so not built (%s); run `make` or __graft_entry__.build()" % LIB_PATH)
        # One HIP runtime per process: torch ships its own libamdhip64 (soname .so.7, file name
        # .so).  Loaded first, it also serves this library's libamdhip64.so.7; loaded after
        # /opt/rocm's copy, it is a second runtime in the process and torch then sees no GPU.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        vp, i, f, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
        sig = {
            "qec_last_error": (ctypes.c_char_p, []),
            "qec_abi_version": (i, []),
            "qec_build_id": (ctypes.c_char_p, []),
            "qec_code_load": (vp, [ctypes.c_char_p]),
            "qec_code_generate": (vp, [i, i, i, i, i, i]),
            "qec_code_from_matrices": (vp, [i, i, vp, i, vp]),
            "qec_code_degrees": (i, [vp, vp]),
            "qec_code_layers": (i, [vp, i, vp]),
            "qec_code_has_wave_minsum": (i, [vp]),
            "qec_code_free": (i, [vp]),
            "qec_code_params": (i, [vp, vp]),
            "qec_code_exponents": (i, [vp, i, vp]),
            "qec_code_pcm": (i, [vp, i, vp]),
            "qec_code_describe": (i, [vp, ctypes.c_char_p, sz]),
            "qec_code_syndrome": (i, [vp, i, vp, sz, vp]),
            "qec_code_check_logical": (i, [vp, vp, vp, sz, vp]),
            "qec_code_with_logical": (vp, [vp, i]),
            "qec_code_logical_mode": (i, [vp]),
            "qec_code_logical_rows": (i, [vp, vp]),
            "qec_code_imp": (i, [vp, vp]),
            "qec_decoder_create": (vp, [vp, i, sz]),
            "qec_decoder_create_engine": (vp, [vp, i, sz, i]),
            "qec_decoder_create_multi": (vp, [vp, vp, i, sz]),
            "qec_decoder_create_multi_engine": (vp, [vp, vp, i, sz, i]),
            "qec_decoder_destroy": (i, [vp]),
            "qec_decoder_num_parts": (i, [vp]),
            "qec_decoder_part": (vp, [vp, i]),
            "qec_decoder_device": (i, [vp]),
            "qec_decoder_describe": (i, [vp, ctypes.c_char_p, sz]),
            "qec_decoder_set_option": (i, [vp, i, i]),
            "qec_decoder_get_option": (i, [vp, i, vp]),
            "qec_near_hard_threshold": (i, [f, i, i, vp, vp]),
            "qec_near_probe": (i, [f, f, f, vp]),
            "qec_decoder_set_priors": (i, [vp, vp, vp]),
            "qec_decoder_get_priors": (i, [vp, vp, vp]),
            "qec_decoder_get_osd_weights": (i, [vp, vp, vp]),
            "qec_sample_independent_dev": (i, [vp, ctypes.c_uint64, ctypes.c_uint64, sz, vp, vp, vp]),
            "qec_correlated_priors": (i, [f, vp, vp]),
            "qec_minsum_llr": (i, [f, vp]),
            "qec_decoder_get_minsum_llr": (i, [vp, vp, vp]),
            "qec_decoder_set_relay": (i, [vp, vp, vp, i, i]),
            "qec_decoder_get_relay": (i, [vp, vp, vp, vp, vp]),
            "qec_decoder_set_syndrome_priors": (i, [vp, vp, vp]),
            "qec_decoder_get_syndrome_priors": (i, [vp, vp, vp]),
            "qec_decode_batch_soft": (i, [vp, vp, vp, sz, f, i, i, vp, vp, vp, vp, vp, vp, vp]),
            "qec_decode_batch_soft_dev": (i, [vp, vp, vp, sz, f, i, i, vp, vp, vp, vp, vp, vp, vp, vp]),
            "qec_flip_syndrome_dev": (i, [vp, ctypes.c_uint64, ctypes.c_uint64, sz, vp, vp, vp, vp, vp]),
            "qec_decoder_set_pauli_channel": (i, [vp, vp, vp, vp]),
            "qec_decoder_get_pauli_channel": (i, [vp, vp, vp, vp]),
            "qec_decoder_get_conditional_priors": (i, [vp, vp, vp, vp, vp]),
            "qec_sample_pauli_dev": (i, [vp, ctypes.c_uint64, ctypes.c_uint64, sz, vp, vp, vp]),
            "qec_decode_batch": (i, [vp, vp, vp, sz, f, i, i, vp, vp, vp, vp, vp]),
            "qec_decode_batch_dev": (i, [vp, vp, vp, sz, f, i, i, vp, vp, vp, vp, vp, vp]),
            "qec_decode_batch_packed": (i, [vp, vp, vp, sz, f, i, i, vp, vp]),
            "qec_decode_batch_packed_dev": (i, [vp, vp, vp, sz, f, i, i, vp, vp, vp, vp]),
            "qec_decode_bits_packed_dev": (i, [vp, vp, vp, sz, f, i, i, vp, vp, vp, vp]),
            "qec_sample_fixed_weight": (i, [ctypes.c_uint32, i, sz, i, vp, vp]),
            "qec_get_statistics": (i, [vp, i, i, f, i, ctypes.c_uint32, i, ctypes.POINTER(Stats)]),
            "qec_sample_depolarizing_dev": (i, [vp, ctypes.c_uint64, ctypes.c_uint64, sz, f, vp, vp, vp]),
            "qec_sample_syndrome_dev": (i, [vp, ctypes.c_uint64, ctypes.c_uint64, sz, f, vp, vp, vp, vp]),
            "qec_syndrome_dev": (i, [vp, vp, vp, sz, vp, vp, vp]),
            "qec_statistics_dev": (i, [vp, vp, vp, vp, vp, vp, sz, vp, vp]),
            "qec_statistics_packed_dev": (i, [vp, vp, vp, vp, sz, vp, vp]),
            "qec_logical_packed_dev": (i, [vp, vp, vp, sz, vp, vp]),
            "qec_pack_decisions_dev": (i, [vp, vp, vp, vp, sz, vp, vp]),
            "qec_osd": (i, [vp, vp, vp, sz, vp, vp, vp, vp]),
            "qec_osd_dev": (i, [vp, vp, vp, sz, vp, vp, vp, vp, vp]),
            "qec_monte_carlo": (i, [vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, f, i, i, sz,
                                    ctypes.POINTER(MCResult)]),
        }
        for name, (res, args) in sig.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def last_error():
    return lib().qec_last_error().decode()


def build_id():
    """Hash of the sources and flags the loaded library was built from (Makefile BUILD_ID)."""
    return lib().qec_build_id().decode()


def near_hard_threshold(p_prime, R, L):
    """qec_near_hard_threshold: (eps0, T) of the near-hard jump for p' (a float32), R checks per variable
    and L variables per check; eps0 = 0.0 means the jump never fires."""
    eps0, T = ctypes.c_float(0.0), ctypes.c_uint32(0)
    _check(lib().qec_near_hard_threshold(float(np.float32(p_prime)), int(R), int(L), ctypes.byref(eps0), ctypes.byref(T)),
           "qec_near_hard_threshold")
    return float(eps0.value), int(T.value)


def near_probe(t0, t1, eps0):
    """qec_near_probe: (passes, side) of the near-hard probe for the folds t0, t1 (float32) of one outgoing
    message t1 / (t0 + t1); side = 1 iff t1 > t0."""
    side = ctypes.c_int(0)
    ok = lib().qec_near_probe(float(np.float32(t0)), float(np.float32(t1)), float(np.float32(eps0)), ctypes.byref(side))
    return bool(ok), int(side.value)


def correlated_priors(p):
    """qec_correlated_priors: (c0, c1) as float32 -- the priors of one sector's bit given that the other sector's
    bit of the same qubit is clear / set, under depolarising noise of strength p (a float32): the scalar tables
    of set_option("correlated", 1 | 2) on a decoder without priors."""
    c0, c1 = ctypes.c_float(0.0), ctypes.c_float(0.0)
    _check(lib().qec_correlated_priors(float(np.float32(p)), ctypes.byref(c0), ctypes.byref(c1)), "qec_correlated_priors")
    return np.float32(c0.value), np.float32(c1.value)


def has_wave_minsum(code):
    """qec_code_has_wave_minsum: whether a sparse-engine decoder of `code` takes set_option("minsum_wave", 1)."""
    return code.has_wave_minsum()


def minsum_llr(prior):
    """qec_minsum_llr: the channel LLR of min-sum BP (set_option("bp_method", 1)) for a prior (a float32), as
    float32: (float) log((1 - prior) / prior) clamped to +-2^30; > 0 means the bit is 0."""
    llr = ctypes.c_float(0.0)
    _check(lib().qec_minsum_llr(float(np.float32(prior)), ctypes.byref(llr)), "qec_minsum_llr")
    return np.float32(llr.value)


def relay_gammas(n, legs, gamma0=0.125, lo=-0.24, hi=0.66, seed=0):
    """Memory strengths for set_relay as float32 [legs, n]: row 0 is gamma0 everywhere, the other rows are
    numpy.random.default_rng(seed).uniform(lo, hi, (legs - 1, n))."""
    g = np.empty((int(legs), int(n)), dtype=np.float32)
    g[0] = gamma0
    g[1:] = np.random.default_rng(seed).uniform(lo, hi, (int(legs) - 1, int(n)))
    return g


def _check(rc, what):
    if rc != 0:
        raise QecError("%s failed (%d): %s" % (what, rc, last_error()))


def _ptr(a):
    if a is None:
        return None
    return a.ctypes.data_as(ctypes.c_void_p)


def syndrome_bytes(s):
    """Integer syndrome entries to the ABI's bytes, keeping both of the reference's readings of an
    entry: its truthiness in the check update (DecoderCPU.h:178) and its exact value in the
    syndrome comparison (:381) -- 0 -> 0, 1 -> 1, anything else -> 2 (as include/Decoder.h)."""
    s = np.asarray(s)
    return np.where(s == 0, 0, np.where(s == 1, 1, 2)).astype(np.uint8)


def _u8(a, shape):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.shape != shape:
        a = a.reshape(shape)
    return a


class Quantum_LDPC_Code:
    """Code model (QEC_LDPC/Quantum_LDPC_Code.h:7-150)."""

    def __init__(self, handle):
        if not handle:
            raise QecError(last_error())
        self._h = ctypes.c_void_p(handle)
        v = np.zeros(9, dtype=np.int32)
        _check(lib().qec_code_params(self._h, _ptr(v)), "qec_code_params")
        (self.J, self.K, self.L, self.P, self.sigma, self.tau, self.n, self.numEqsX,
         self.numEqsZ) = (int(x) for x in v)
        # slots per check of the message / q_final layout: L, or D of a general code (degrees()[4])
        self.stride = self.L if self.L else self.degrees()[4]

    @staticmethod
    def createFromFile(path):
        h = lib().qec_code_load(os.fsencode(path))
        if not h:
            raise QecError(last_error())
        return Quantum_LDPC_Code(h)

    load = createFromFile

    @staticmethod
    def createFromMatrices(HX, HZ):
        """A general CSS code from its two 0/1 parity-check matrices (qec_code_from_matrices): any row
        and column weights, HX [mX, n] and HZ [mZ, n].  J = K = L = P = sigma = tau = 0; with_logical
        derives its logical check."""
        HX, HZ = np.asarray(HX), np.asarray(HZ)
        if HX.ndim != 2 or HZ.ndim != 2 or HX.shape[1] != HZ.shape[1]:
            raise QecError("createFromMatrices: HX and HZ must be 2-D with the same number of columns")
        for name, H in (("HX", HX), ("HZ", HZ)):
            bad = np.argwhere((H != 0) & (H != 1))
            if len(bad):  # before the cast to bytes folds the value
                r, v = (int(x) for x in bad[0])
                raise QecError("createFromMatrices: %s[%d][%d] = %r is not 0 or 1" % (name, r, v, H[r, v].item()))
        hx = np.ascontiguousarray(HX, dtype=np.uint8)
        hz = np.ascontiguousarray(HZ, dtype=np.uint8)
        h = lib().qec_code_from_matrices(hx.shape[1], hx.shape[0], _ptr(hx), hz.shape[0], _ptr(hz))
        if not h:
            raise QecError(last_error())
        return Quantum_LDPC_Code(h)

    def degrees(self):
        """(max row weight X, max row weight Z, max column weight X, max column weight Z, slot stride D)
        (qec_code_degrees); a regular code gives (L, L, J, K, L)."""
        v = np.zeros(5, dtype=np.int32)
        _check(lib().qec_code_degrees(self._h, _ptr(v)), "qec_code_degrees")
        return tuple(int(x) for x in v)

    def has_wave_minsum(self):
        """Whether set_option("minsum_wave", 1) has kernels for this code (qec_code_has_wave_minsum): a
        circulant-permutation code with P <= 64 and a block shape of the runtime-shift table.  A host query."""
        r = lib().qec_code_has_wave_minsum(self._h)
        if r < 0:
            raise QecError("qec_code_has_wave_minsum failed: %s" % last_error())
        return bool(r)

    def layers(self, sector):
        """The colour of every check of the sector under the serial BP schedule (qec_code_layers): int32
        [numEqs]; checks of one colour share no variable, and the processing order is (colour, index)."""
        sector = int(sector)
        colour = np.zeros(self.numEqsZ if sector else self.numEqsX, dtype=np.int32)
        if lib().qec_code_layers(self._h, sector, _ptr(colour)) < 0:
            raise QecError("qec_code_layers failed: %s" % last_error())
        return colour

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:
            _lib.qec_code_free(h)
            self._h = None

    @property
    def handle(self):
        return self._h

    def describe(self):
        buf = ctypes.create_string_buffer(256)
        _check(lib().qec_code_describe(self._h, buf, 256), "qec_code_describe")
        return buf.value.decode()

    __str__ = describe

    def exponents(self, sector):
        R = self.K if sector else self.J
        e = np.zeros((R, self.L), dtype=np.int32)
        _check(lib().qec_code_exponents(self._h, int(sector), _ptr(e)), "qec_code_exponents")
        return e

    def pcm(self, sector):
        m = self.numEqsZ if sector else self.numEqsX
        h = np.zeros((m, self.n), dtype=np.uint8)
        _check(lib().qec_code_pcm(self._h, int(sector), _ptr(h)), "qec_code_pcm")
        return h

    @property
    def pcmX(self):
        return self.pcm(0)

    @property
    def pcmZ(self):
        return self.pcm(1)

    def syndrome(self, sector, errors):
        """Batched GetSyndromeX/Z: errors [B, n] -> [B, m]."""
        e = np.atleast_2d(np.ascontiguousarray(errors, dtype=np.uint8))
        m = self.numEqsZ if sector else self.numEqsX
        s = np.empty((e.shape[0], m), dtype=np.uint8)
        _check(lib().qec_code_syndrome(self._h, int(sector), _ptr(e), e.shape[0], _ptr(s)), "qec_code_syndrome")
        return s

    def GetSyndromeX(self, errors):
        return self.syndrome(0, errors)[0]

    def GetSyndromeZ(self, errors):
        return self.syndrome(1, errors)[0]

    def check_logical(self, ex, ez):
        ex = np.atleast_2d(np.ascontiguousarray(ex, dtype=np.uint8))
        ez = np.atleast_2d(np.ascontiguousarray(ez, dtype=np.uint8))
        out = np.empty(ex.shape[0], dtype=np.uint8)
        _check(lib().qec_code_check_logical(self._h, _ptr(ex), _ptr(ez), ex.shape[0], _ptr(out)),
               "qec_code_check_logical")
        return out.astype(bool)

    def CheckLogicalError(self, errors):
        errors = np.asarray(errors)
        return bool(self.check_logical(errors[: self.n], errors[self.n:])[0])

    def with_logical(self, mode):
        """A new code with the same matrices whose logical check is derived from them
        (qec_code_with_logical): "reference" = rx not in rowspace(pcmX) or rz not in rowspace(pcmZ),
        what the shipped I-P files compute; "degenerate" = rx not in rowspace(pcmZ) or rz not in
        rowspace(pcmX), a residual that is a product of stabilizers counts as corrected (needs
        pcmX pcmZ^T = 0).  This code is unchanged."""
        if mode not in ("reference", "degenerate"):
            raise QecError("with_logical: mode must be 'reference' or 'degenerate', not %r" % (mode,))
        h = lib().qec_code_with_logical(self._h, LOGICAL[mode])
        if not h:
            raise QecError(last_error())
        return Quantum_LDPC_Code(h)

    @property
    def logical_mode(self):
        """"file" (the code file's I-P matrix, or no check at all), "reference" or "degenerate"."""
        v = lib().qec_code_logical_mode(self._h)
        return {b: a for a, b in LOGICAL.items()}[v]

    @property
    def logical_rows(self):
        """Non-zero rows of the logical check's matrix (0: the code has none)."""
        v = ctypes.c_int(0)
        _check(lib().qec_code_logical_rows(self._h, ctypes.byref(v)), "qec_code_logical_rows")
        return v.value

    def imp(self):
        """The dense 2n x 2n I-P matrix (the file's, or the derived one)."""
        a = np.zeros((2 * self.n, 2 * self.n), dtype=np.uint8)
        _check(lib().qec_code_imp(self._h, _ptr(a)), "qec_code_imp")
        return a


def QC_LDPC_CSS(J, K, L, P, sigma, tau):
    """Generated code (QEC_LDPC/QEC_LDPC_CSS.cu:5-131); carries no I-P matrix (with_logical derives
    the check)."""
    h = lib().qec_code_generate(J, K, L, P, sigma, tau)
    if not h:
        raise QecError(last_error())
    return Quantum_LDPC_Code(h)


def sample_fixed_weight(seed, W, count, n):
    """The reference's fixed-weight sampler stream (DecoderCPU.h:448-459)."""
    x = np.empty((count, n), dtype=np.uint8)
    z = np.empty((count, n), dtype=np.uint8)
    _check(lib().qec_sample_fixed_weight(seed & 0xFFFFFFFF, W, count, n, _ptr(x), _ptr(z)),
           "qec_sample_fixed_weight")
    return x, z


class DecoderGPU:
    """MI355X BP engine behind the reference's DecoderGPU slot (QEC_LDPC/DecoderGPU.h).

    engine: "auto" (wave-circulant kernel when the code has one, else sparse-graph),
    "circulant" or "sparse" (include/qec_ldpc.h, QEC_ENGINE_*).
    max_batch: sizes the device-pointer workspace so the *_dev decodes allocate nothing for
    batches up to it (graph capture); larger batches grow it on demand.
    devices: a list of HIP device ordinals for a multi-device decoder (qec_decoder_create_multi_engine, every part
    on `engine`):
    the host-buffer calls, GetStatistics and monte_carlo shard their samples over the devices;
    the *_dev calls go to one of parts()."""

    def __init__(self, code, device=0, engine="auto", max_batch=0, devices=None, _handle=None):
        self.code = code
        self._owned = _handle is None
        if _handle is not None:
            h = _handle
        elif devices is not None:
            devs = (ctypes.c_int * len(devices))(*[int(x) for x in devices])
            h = lib().qec_decoder_create_multi_engine(code.handle, devs, len(devices), int(max_batch), ENGINE[engine])
        else:
            h = lib().qec_decoder_create_engine(code.handle, int(device), int(max_batch), ENGINE[engine])
        if not h:
            raise QecError(last_error())
        self._h = ctypes.c_void_p(h)
        self.device = int(lib().qec_decoder_device(self._h))
        self.num_parts = int(lib().qec_decoder_num_parts(self._h))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None and getattr(self, "_owned", False):
            _lib.qec_decoder_destroy(h)
        self._h = None

    def parts(self):
        """Single-device views of a multi-device decoder's parts (or [self])."""
        if self.num_parts == 1:
            return [self]
        out = []
        for k in range(self.num_parts):
            h = lib().qec_decoder_part(self._h, k)
            if not h:
                raise QecError(last_error())
            p = DecoderGPU(self.code, _handle=h)
            p._parent = self  # keeps the group (the owner of the part) alive
            out.append(p)
        return out

    def describe(self):
        buf = ctypes.create_string_buffer(256)
        _check(lib().qec_decoder_describe(self._h, buf, 256), "qec_decoder_describe")
        return buf.value.decode()

    def set_option(self, name, value):
        """qec_decoder_set_option (include/qec_ldpc.h): e.g. set_option("hard_paths", 0)."""
        _check(lib().qec_decoder_set_option(self._h, OPTION[name], int(value)), "qec_decoder_set_option")

    def get_option(self, name):
        v = ctypes.c_int(0)
        _check(lib().qec_decoder_get_option(self._h, OPTION[name], ctypes.byref(v)), "qec_decoder_get_option")
        return v.value

    def set_priors(self, priorX, priorZ):
        """Per-qubit priors (qec_decoder_set_priors): priorX[v] / priorZ[v] is the prior that bit v of eX / eZ
        is 1 -- array-likes of length n (float32 values are taken as they are), or a scalar for every qubit;
        set_priors(None, None) clears them.  While set, BP uses them in place of p' = (2/3) p and the `p`
        argument of every decode call, GetStatistics, sample_syndrome_dev and monte_carlo is not used (the
        latter two draw sample_independent_dev's errors).  Sparse-graph and CPU engines; a wave-circulant
        decoder refuses (create it with engine="sparse").  OSD-CS scores its candidates by Hamming weight
        unless set_option("osd_score", 1) asks for the prior-weighted score; every set rebuilds the weight
        tables that score reads (osd_weights)."""
        if (priorX is None) != (priorZ is None):
            raise QecError("set_priors: priorX and priorZ must both be given, or both be None (clear)")
        if priorX is None:
            _check(lib().qec_decoder_set_priors(self._h, None, None), "qec_decoder_set_priors")
            return
        arrs = []
        for name, pr in (("priorX", priorX), ("priorZ", priorZ)):
            a = np.asarray(pr, dtype=np.float32)
            if a.ndim == 0:
                a = np.full(self.code.n, a, dtype=np.float32)
            if a.shape != (self.code.n,):
                raise QecError("set_priors: %s must be a scalar or have length n = %d, has shape %s"
                               % (name, self.code.n, a.shape))
            arrs.append(np.ascontiguousarray(a))
        _check(lib().qec_decoder_set_priors(self._h, _ptr(arrs[0]), _ptr(arrs[1])), "qec_decoder_set_priors")

    def get_priors(self):
        """(priorX, priorZ) as float32 arrays (qec_decoder_get_priors), or None when no priors are set."""
        pX = np.empty(self.code.n, dtype=np.float32)
        pZ = np.empty(self.code.n, dtype=np.float32)
        rc = lib().qec_decoder_get_priors(self._h, _ptr(pX), _ptr(pZ))
        if rc < 0:
            raise QecError("qec_decoder_get_priors failed (%d): %s" % (rc, last_error()))
        return (pX, pZ) if rc == 1 else None

    def set_pauli_channel(self, pX, pY, pZ):
        """Per-qubit Pauli channel (qec_decoder_set_pauli_channel): qubit v suffers X, Y or Z with probabilities
        pX[v], pY[v], pZ[v] (Y sets both bits) -- array-likes of length n or scalars for every qubit;
        set_pauli_channel(None, None, None) clears the channel and the priors.  Installs the marginals pX + pY and
        pZ + pY as set_priors does (get_priors returns them), the conditional tables that
        set_option("correlated", 1 | 2) decodes the second sector with (get_conditional_priors), and the noise
        that sample_pauli_dev, sample_syndrome_dev and monte_carlo draw.  A later set_priors drops the channel."""
        given = [a is not None for a in (pX, pY, pZ)]
        if not any(given):
            _check(lib().qec_decoder_set_pauli_channel(self._h, None, None, None), "qec_decoder_set_pauli_channel")
            return
        if not all(given):
            raise QecError("set_pauli_channel: pX, pY and pZ must all be given, or all be None (clear)")
        arrs = []
        for name, pr in (("pX", pX), ("pY", pY), ("pZ", pZ)):
            a = np.asarray(pr, dtype=np.float32)
            if a.ndim == 0:
                a = np.full(self.code.n, a, dtype=np.float32)
            if a.shape != (self.code.n,):
                raise QecError("set_pauli_channel: %s must be a scalar or have length n = %d, has shape %s"
                               % (name, self.code.n, a.shape))
            arrs.append(np.ascontiguousarray(a))
        _check(lib().qec_decoder_set_pauli_channel(self._h, *[_ptr(a) for a in arrs]), "qec_decoder_set_pauli_channel")

    def _get_tables(self, fn, count):
        out = [np.empty(self.code.n, dtype=np.float32) for _ in range(count)]
        rc = getattr(lib(), fn)(self._h, *[_ptr(a) for a in out])
        if rc < 0:
            raise QecError("%s failed (%d): %s" % (fn, rc, last_error()))
        return tuple(out) if rc == 1 else None

    def get_pauli_channel(self):
        """(pX, pY, pZ) as float32 arrays (qec_decoder_get_pauli_channel), or None when no channel is set."""
        return self._get_tables("qec_decoder_get_pauli_channel", 3)

    def get_conditional_priors(self):
        """(cZ0, cZ1, cX0, cX1) as float32 arrays (qec_decoder_get_conditional_priors): the prior of a qubit's Z
        bit given its X bit clear / set, and of its X bit given its Z bit clear / set, under the Pauli channel;
        None when no channel is set."""
        return self._get_tables("qec_decoder_get_conditional_priors", 4)

    def osd_weights(self):
        """(wX, wZ) as int32 arrays (qec_decoder_get_osd_weights): the integer weights, 0 .. 4095 in
        sixteenths of a bit of log-likelihood ratio, that OSD-CS sums over a candidate's flips under
        set_option("osd_score", 1); None when no priors are set."""
        wX = np.empty(self.code.n, dtype=np.int32)
        wZ = np.empty(self.code.n, dtype=np.int32)
        rc = lib().qec_decoder_get_osd_weights(self._h, _ptr(wX), _ptr(wZ))
        if rc < 0:
            raise QecError("qec_decoder_get_osd_weights failed (%d): %s" % (rc, last_error()))
        return (wX, wZ) if rc == 1 else None

    def minsum_llr(self):
        """(llrX, llrZ) as float32 arrays (qec_decoder_get_minsum_llr): the channel LLRs of the handle's priors,
        which min-sum BP (set_option("bp_method", 1)) decodes under; raises QecError when no priors are set."""
        lX = np.empty(self.code.n, dtype=np.float32)
        lZ = np.empty(self.code.n, dtype=np.float32)
        _check(lib().qec_decoder_get_minsum_llr(self._h, _ptr(lX), _ptr(lZ)), "qec_decoder_get_minsum_llr")
        return lX, lZ

    def set_relay(self, gammaX, gammaZ, solutions=1):
        """Relay-BP (qec_decoder_set_relay): min-sum with one memory per variable, run as a chain of legs that stops at
        the first solution or at the lightest of the first `solutions` ones.  gammaX / gammaZ: the memory strengths,
        |gamma| <= 1 -- arrays of shape [legs, n], an [n] array for one leg, or a scalar for one uniform leg;
        set_relay(None, None) clears.  In effect in every decode while set_option("bp_method", 1); relay_gammas makes
        tables.  Sparse-graph and CPU engines; a wave-circulant decoder refuses (create it with engine="sparse")."""
        if (gammaX is None) != (gammaZ is None):
            raise QecError("set_relay: gammaX and gammaZ must both be given, or both be None (clear)")
        if gammaX is None:
            _check(lib().qec_decoder_set_relay(self._h, None, None, 0, 0), "qec_decoder_set_relay")
            return
        arrs = []
        for name, g in (("gammaX", gammaX), ("gammaZ", gammaZ)):
            a = np.asarray(g, dtype=np.float32)
            if a.ndim == 0:
                a = np.full((1, self.code.n), a, dtype=np.float32)
            if a.ndim == 1:
                a = a[None, :]
            if a.ndim != 2 or a.shape[1] != self.code.n:
                raise QecError("set_relay: %s must be a scalar, or have shape [n] or [legs, n] with n = %d, has shape %s"
                               % (name, self.code.n, a.shape))
            arrs.append(np.ascontiguousarray(a))
        if arrs[0].shape != arrs[1].shape:
            raise QecError("set_relay: gammaX and gammaZ must have the same number of legs")
        _check(lib().qec_decoder_set_relay(self._h, _ptr(arrs[0]), _ptr(arrs[1]), arrs[0].shape[0], int(solutions)),
               "qec_decoder_set_relay")

    def get_relay(self):
        """(gammaX, gammaZ, solutions) with float32 tables [legs, n] (qec_decoder_get_relay), or None without tables."""
        legs, sol = ctypes.c_int(0), ctypes.c_int(0)
        _check(lib().qec_decoder_get_relay(self._h, None, None, ctypes.byref(legs), ctypes.byref(sol)), "qec_decoder_get_relay")
        if legs.value == 0:
            return None
        gX = np.empty((legs.value, self.code.n), dtype=np.float32)
        gZ = np.empty((legs.value, self.code.n), dtype=np.float32)
        _check(lib().qec_decoder_get_relay(self._h, _ptr(gX), _ptr(gZ), None, None), "qec_decoder_get_relay")
        return gX, gZ, sol.value

    def set_syndrome_priors(self, qX, qZ):
        """Noisy syndromes (qec_decoder_set_syndrome_priors): qX [numEqsX], qZ [numEqsZ] = the probability that each
        check's measured bit is flipped (arrays, or a scalar for every check); (None, None) clears.  Every min-sum decode
        of the handle then treats the syndrome bits as soft: decode_batch(..., want_flips=True) also returns which
        measured bits the decoder took as flipped.  Needs set_option("bp_method", 1); refused beside relay tables
        and "osd" = 1, and by a wave-circulant decoder."""
        if (qX is None) != (qZ is None):
            raise QecError("set_syndrome_priors: qX and qZ must both be given, or both be None (clear)")
        if qX is None:
            _check(lib().qec_decoder_set_syndrome_priors(self._h, None, None), "qec_decoder_set_syndrome_priors")
            return
        arrs = []
        for name, q, m in (("qX", qX, self.code.numEqsX), ("qZ", qZ, self.code.numEqsZ)):
            a = np.asarray(q, dtype=np.float32)
            if a.ndim == 0:
                a = np.full(m, a, dtype=np.float32)
            if a.shape != (m,):
                raise QecError("set_syndrome_priors: %s must be a scalar or have shape [%d], has shape %s" % (name, m, a.shape))
            arrs.append(np.ascontiguousarray(a))
        _check(lib().qec_decoder_set_syndrome_priors(self._h, _ptr(arrs[0]), _ptr(arrs[1])),
               "qec_decoder_set_syndrome_priors")

    def get_syndrome_priors(self):
        """(qX, qZ) as float32 arrays (qec_decoder_get_syndrome_priors), or None when none are set."""
        qX = np.empty(self.code.numEqsX, dtype=np.float32)
        qZ = np.empty(self.code.numEqsZ, dtype=np.float32)
        rc = lib().qec_decoder_get_syndrome_priors(self._h, _ptr(qX), _ptr(qZ))
        if rc < 0:
            raise QecError("qec_decoder_get_syndrome_priors failed (%d): %s" % (rc, last_error()))
        return (qX, qZ) if rc == 1 else None

    def last_path(self):
        """The launch sequence of this handle's last decode call (QEC_OPT_LAST_PATH) as a set of
        PATH names, e.g. {"bit_rows", "records", "ordered", "sector_order", "sector_launches"}."""
        v = self.get_option("last_path")
        return {k for k, b in PATH.items() if v & b}

    def record_bytes(self):
        """Bytes of one packed decision record: 2 ceil(n/8) + 1."""
        return record_bytes(self.code.n)

    # ---- host buffers ------------------------------------------------------------------
    def decode_batch(self, sX, sZ, p, max_iter, stop="ref", want_iters=False, want_q=False, want_flips=False):
        """Host-buffer batch decode -> (eX, eZ, flags, iters|None, q|None).  With priors set (set_priors)
        BP uses them and p is not used, here and in every other decode call.  want_flips (a min-sum handle;
        qec_decode_batch_soft): two further items fX [B, numEqsX], fZ [B, numEqsZ], the measured syndrome bits the
        decoder took as flipped (all zero without set_syndrome_priors)."""
        c = self.code
        sX = np.atleast_2d(sX)
        B = sX.shape[0]
        sX = _u8(sX, (B, c.numEqsX))
        sZ = _u8(sZ, (B, c.numEqsZ))
        eX = np.empty((B, c.n), dtype=np.uint8)
        eZ = np.empty((B, c.n), dtype=np.uint8)
        flags = np.empty(B, dtype=np.uint8)
        iters = np.empty((B, 2), dtype=np.int32) if want_iters else None
        q = np.empty((B, (c.numEqsX + c.numEqsZ) * c.stride), dtype=np.float32) if want_q else None
        if want_flips:
            fX = np.empty((B, c.numEqsX), dtype=np.uint8)
            fZ = np.empty((B, c.numEqsZ), dtype=np.uint8)
            _check(lib().qec_decode_batch_soft(self._h, _ptr(sX), _ptr(sZ), B, float(p), int(max_iter), STOP[stop],
                                               _ptr(eX), _ptr(eZ), _ptr(fX), _ptr(fZ), _ptr(flags), _ptr(iters), _ptr(q)),
                   "qec_decode_batch_soft")
            return eX, eZ, flags, iters, q, fX, fZ
        _check(lib().qec_decode_batch(self._h, _ptr(sX), _ptr(sZ), B, float(p), int(max_iter), STOP[stop],
                                      _ptr(eX), _ptr(eZ), _ptr(flags), _ptr(iters), _ptr(q)), "qec_decode_batch")
        return eX, eZ, flags, iters, q

    def decode_batch_packed(self, sX, sZ, p, max_iter, stop="ref", want_iters=False):
        """Host-buffer batch decode to packed decision records -> (records [B, record_bytes()], iters|None)."""
        c = self.code
        sX = np.atleast_2d(sX)
        B = sX.shape[0]
        sX = _u8(sX, (B, c.numEqsX))
        sZ = _u8(sZ, (B, c.numEqsZ))
        rec = np.empty((B, self.record_bytes()), dtype=np.uint8)
        iters = np.empty((B, 2), dtype=np.int32) if want_iters else None
        _check(lib().qec_decode_batch_packed(self._h, _ptr(sX), _ptr(sZ), B, float(p), int(max_iter), STOP[stop],
                                             _ptr(rec), _ptr(iters)), "qec_decode_batch_packed")
        return rec, iters

    def osd(self, sX, sZ, q, eX, eZ, flags):
        """OSD (qec_osd) on a decoded host batch: q is the soft input in decode_batch's q layout.
        Returns repaired copies (eX, eZ, flags); sectors without their SYNDROME_FAIL bit are untouched.
        set_option("osd_order", lam) chooses OSD-0 (0, the default) or the combination sweep OSD-CS over
        the lam <= 64 most suspicious non-pivot columns; get_option("osd_sectors") / ("osd_cs_sectors")
        then give the sectors repaired and those whose lightest candidate was not the OSD-0 estimate.
        With priors set, set_option("osd_score", 1) makes the sweep pick the candidate of least
        prior-weighted score (osd_weights) instead of the lightest; the default 0 is Hamming weight."""
        c = self.code
        sX = np.atleast_2d(sX)
        B = sX.shape[0]
        sX = _u8(sX, (B, c.numEqsX))
        sZ = _u8(sZ, (B, c.numEqsZ))
        q = np.ascontiguousarray(q, dtype=np.float32).reshape(B, (c.numEqsX + c.numEqsZ) * c.stride)
        eX = _u8(eX, (B, c.n)).copy()
        eZ = _u8(eZ, (B, c.n)).copy()
        flags = _u8(flags, (B,)).copy()
        _check(lib().qec_osd(self._h, _ptr(sX), _ptr(sZ), B, _ptr(q), _ptr(eX), _ptr(eZ), _ptr(flags)), "qec_osd")
        return eX, eZ, flags

    # ---- device buffers (torch tensors on this decoder's GPU) ---------------------------
    _binding = False

    def _issue(self, name, args):
        """Calls the C entry point, or (inside bind) returns it with its checked arguments."""
        fn = getattr(lib(), name)
        if self._binding:
            return fn, args, name
        _check(fn(*args), name)

    def bind(self, method, *args, **kw):
        """A zero-argument callable that re-issues one device-buffer decode call (decode_batch_dev,
        decode_batch_packed_dev or decode_bits_packed_dev) with these arguments: the tensors are
        validated and their pointers taken once, so each call is only the C ABI call (for launch-bound
        loops over the same buffers; the tensors must stay alive and unmoved)."""
        self._binding = True
        try:
            fn, cargs, name = method(*args, **kw)
        finally:
            self._binding = False

        def call():
            rc = fn(*cargs)
            if rc != 0:
                raise QecError("%s failed (%d): %s" % (name, rc, last_error()))
        return call

    def _stream(self, stream):
        if stream is None:
            import torch
            return torch.cuda.current_stream(self.device).cuda_stream
        return stream if isinstance(stream, int) else stream.cuda_stream

    def _t(self, t, name, dtype, shape, optional=False):
        """Device pointer of tensor t after checking it is what the C ABI will read or write."""
        if t is None:
            if optional:
                return None
            raise QecError("%s: tensor required" % name)
        import torch
        if not isinstance(t, torch.Tensor):
            raise QecError("%s: expected a torch tensor, got %s" % (name, type(t).__name__))
        if not t.is_cuda or t.device.index != self.device:
            raise QecError("%s: must be on cuda:%d (the decoder's device), is on %s" % (name, self.device, t.device))
        if t.dtype != dtype:
            raise QecError("%s: dtype must be %s, is %s" % (name, dtype, t.dtype))
        if not t.is_contiguous():
            raise QecError("%s: must be contiguous" % name)
        if tuple(t.shape) != tuple(shape):
            raise QecError("%s: shape must be %s, is %s" % (name, tuple(shape), tuple(t.shape)))
        return t.data_ptr()

    def _single(self, what):
        if self.num_parts != 1:
            raise QecError("%s: device buffers live on one GPU; call it on one of parts()" % what)

    def decode_batch_dev(self, sX, sZ, p, max_iter, stop, eX, eZ, flags, iters=None, q=None, stream=None):
        """Device-buffer batch decode on torch tensors, async on `stream` (a torch.cuda.Stream, a raw
        hipStream_t int, or None = torch's current stream on the decoder's device)."""
        import torch
        self._single("decode_batch_dev")
        c = self.code
        B = sX.shape[0]
        u8 = torch.uint8
        args = (self._t(sX, "sX", u8, (B, c.numEqsX)), self._t(sZ, "sZ", u8, (B, c.numEqsZ)),
                B, float(p), int(max_iter), STOP[stop],
                self._t(eX, "eX", u8, (B, c.n)), self._t(eZ, "eZ", u8, (B, c.n)), self._t(flags, "flags", u8, (B,)),
                self._t(iters, "iters", torch.int32, (B, 2), True),
                self._t(q, "q", torch.float32, (B, (c.numEqsX + c.numEqsZ) * c.stride), True))
        return self._issue("qec_decode_batch_dev", (self._h, *args, ctypes.c_void_p(self._stream(stream))))

    def decode_batch_soft_dev(self, sX, sZ, p, max_iter, stop, eX, eZ, flags, fX=None, fZ=None, iters=None, q=None,
                              stream=None):
        """decode_batch_dev of a min-sum handle with the measurement decisions of set_syndrome_priors as optional
        outputs fX [B, numEqsX], fZ [B, numEqsZ] (uint8; all zero without syndrome priors).  No allocation
        (graph-capturable)."""
        import torch
        self._single("decode_batch_soft_dev")
        c = self.code
        B = sX.shape[0]
        u8 = torch.uint8
        args = (self._t(sX, "sX", u8, (B, c.numEqsX)), self._t(sZ, "sZ", u8, (B, c.numEqsZ)),
                B, float(p), int(max_iter), STOP[stop],
                self._t(eX, "eX", u8, (B, c.n)), self._t(eZ, "eZ", u8, (B, c.n)),
                self._t(fX, "fX", u8, (B, c.numEqsX), True), self._t(fZ, "fZ", u8, (B, c.numEqsZ), True),
                self._t(flags, "flags", u8, (B,)),
                self._t(iters, "iters", torch.int32, (B, 2), True),
                self._t(q, "q", torch.float32, (B, (c.numEqsX + c.numEqsZ) * c.stride), True))
        return self._issue("qec_decode_batch_soft_dev", (self._h, *args, ctypes.c_void_p(self._stream(stream))))

    def flip_syndrome_dev(self, seed, start, sX, sZ, fX=None, fZ=None, stream=None):
        """The measurement-error channel of set_syndrome_priors, in place on device byte syndromes of samples
        [start, start + B) (qec_flip_syndrome_dev): X check c is flipped iff word c of sample b's Philox stream
        < floor(qX[c] 2^32), Z check c from word numEqsX + c; fX / fZ (optional) receive the flips."""
        import torch
        self._single("flip_syndrome_dev")
        c = self.code
        B = sX.shape[0]
        u8 = torch.uint8
        _check(lib().qec_flip_syndrome_dev(self._h, seed & (2 ** 64 - 1), start, B,
                                           self._t(sX, "sX", u8, (B, c.numEqsX)), self._t(sZ, "sZ", u8, (B, c.numEqsZ)),
                                           self._t(fX, "fX", u8, (B, c.numEqsX), True),
                                           self._t(fZ, "fZ", u8, (B, c.numEqsZ), True),
                                           ctypes.c_void_p(self._stream(stream))), "qec_flip_syndrome_dev")

    def decode_batch_packed_dev(self, sX, sZ, p, max_iter, stop, records, iters=None, q=None, stream=None):
        """Device-buffer batch decode into packed decision records [B, record_bytes()] (uint8)."""
        import torch
        self._single("decode_batch_packed_dev")
        c = self.code
        B = sX.shape[0]
        u8 = torch.uint8
        args = (self._t(sX, "sX", u8, (B, c.numEqsX)), self._t(sZ, "sZ", u8, (B, c.numEqsZ)),
                B, float(p), int(max_iter), STOP[stop],
                self._t(records, "records", u8, (B, self.record_bytes())),
                self._t(iters, "iters", torch.int32, (B, 2), True),
                self._t(q, "q", torch.float32, (B, (c.numEqsX + c.numEqsZ) * c.stride), True))
        return self._issue("qec_decode_batch_packed_dev", (self._h, *args, ctypes.c_void_p(self._stream(stream))))

    def decode_bits_packed_dev(self, sXbits, sZbits, p, max_iter, stop, records, iters=None, q=None, stream=None):
        """Device-buffer decode of bit-row syndromes (int32 [B, ceil(m/32)] words, bit c of a row =
        check c) into packed decision records [B, record_bytes()] (uint8)."""
        import torch
        self._single("decode_bits_packed_dev")
        c = self.code
        B = sXbits.shape[0]
        args = (self._t(sXbits, "sXbits", torch.int32, (B, (c.numEqsX + 31) // 32)),
                self._t(sZbits, "sZbits", torch.int32, (B, (c.numEqsZ + 31) // 32)),
                B, float(p), int(max_iter), STOP[stop],
                self._t(records, "records", torch.uint8, (B, self.record_bytes())),
                self._t(iters, "iters", torch.int32, (B, 2), True),
                self._t(q, "q", torch.float32, (B, (c.numEqsX + c.numEqsZ) * c.stride), True))
        return self._issue("qec_decode_bits_packed_dev", (self._h, *args, ctypes.c_void_p(self._stream(stream))))

    def osd_dev(self, sX, sZ, q, eX, eZ, flags, stream=None):
        """OSD (qec_osd_dev) in place on a decoded device batch: repairs the sectors of eX / eZ whose
        SYNDROME_FAIL bit is set in flags from the soft input q (decode_batch_dev's q layout) and clears
        the bit.  The handle's "osd_order" option (read at the call) chooses OSD-0 or the combination
        sweep, and "osd_score" (read at the call too) whether, with priors set, the sweep scores by the
        prior-weighted sum (1) or by Hamming weight (0, the default).  Async on `stream`; no allocation (graph-capturable); updates neither "osd_sectors" nor
        "osd_cs_sectors"."""
        import torch
        self._single("osd_dev")
        c = self.code
        B = sX.shape[0]
        u8 = torch.uint8
        args = (self._t(sX, "sX", u8, (B, c.numEqsX)), self._t(sZ, "sZ", u8, (B, c.numEqsZ)), B,
                self._t(q, "q", torch.float32, (B, (c.numEqsX + c.numEqsZ) * c.stride)),
                self._t(eX, "eX", u8, (B, c.n)), self._t(eZ, "eZ", u8, (B, c.n)), self._t(flags, "flags", u8, (B,)))
        return self._issue("qec_osd_dev", (self._h, *args, ctypes.c_void_p(self._stream(stream))))

    def sample_depolarizing_dev(self, seed, start, p, x, z, stream=None):
        """Device depolarising errors (the gap walk over Philox4x32-10 words, include/qec_ldpc.h)
        for samples [start, start + x.shape[0])."""
        import torch
        self._single("sample_depolarizing_dev")
        B, n = x.shape[0], self.code.n
        _check(lib().qec_sample_depolarizing_dev(self._h, seed & (2 ** 64 - 1), start, B, float(p),
                                                 self._t(x, "x", torch.uint8, (B, n)),
                                                 self._t(z, "z", torch.uint8, (B, n)),
                                                 ctypes.c_void_p(self._stream(stream))),
               "qec_sample_depolarizing_dev")

    def sample_independent_dev(self, seed, start, x, z, stream=None):
        """Device errors drawn independently per qubit and sector with the decoder's priors
        (qec_sample_independent_dev; needs set_priors) for samples [start, start + x.shape[0]):
        x[b, v] = word 2v of sample b's Philox stream < floor(priorX[v] 2^32), z[b, v] likewise from
        word 2v + 1 and priorZ."""
        import torch
        self._single("sample_independent_dev")
        B, n = x.shape[0], self.code.n
        _check(lib().qec_sample_independent_dev(self._h, seed & (2 ** 64 - 1), start, B,
                                                self._t(x, "x", torch.uint8, (B, n)),
                                                self._t(z, "z", torch.uint8, (B, n)),
                                                ctypes.c_void_p(self._stream(stream))),
               "qec_sample_independent_dev")

    def sample_pauli_dev(self, seed, start, x, z, stream=None):
        """Device errors of the decoder's Pauli channel (qec_sample_pauli_dev; needs set_pauli_channel) for
        samples [start, start + x.shape[0]): word u of qubit v is output word v % 4 of sample b's Philox call
        v // 4; x[b, v] = u < tXY[v], z[b, v] = tX[v] <= u < tXYZ[v]."""
        import torch
        self._single("sample_pauli_dev")
        B, n = x.shape[0], self.code.n
        _check(lib().qec_sample_pauli_dev(self._h, seed & (2 ** 64 - 1), start, B,
                                          self._t(x, "x", torch.uint8, (B, n)),
                                          self._t(z, "z", torch.uint8, (B, n)),
                                          ctypes.c_void_p(self._stream(stream))),
               "qec_sample_pauli_dev")

    def sample_syndrome_dev(self, seed, start, p, sX, sZ, errp=None, stream=None):
        """Fused front end: syndromes of the depolarising errors of samples [start, start + B)
        (the sample_depolarizing_dev stream), optionally the errors bit-packed (errp [B, 2 ceil(n/8)]).
        With priors set the errors are sample_independent_dev's and p is not used."""
        import torch
        self._single("sample_syndrome_dev")
        c = self.code
        B = sX.shape[0]
        _check(lib().qec_sample_syndrome_dev(self._h, seed & (2 ** 64 - 1), start, B, float(p),
                                             self._t(sX, "sX", torch.uint8, (B, c.numEqsX)),
                                             self._t(sZ, "sZ", torch.uint8, (B, c.numEqsZ)),
                                             self._t(errp, "errp", torch.uint8, (B, 2 * ((c.n + 7) // 8)), True),
                                             ctypes.c_void_p(self._stream(stream))), "qec_sample_syndrome_dev")

    def syndrome_dev(self, x, z, sX, sZ, stream=None):
        import torch
        self._single("syndrome_dev")
        c = self.code
        B = x.shape[0]
        u8 = torch.uint8
        _check(lib().qec_syndrome_dev(self._h, self._t(x, "x", u8, (B, c.n)), self._t(z, "z", u8, (B, c.n)), B,
                                      self._t(sX, "sX", u8, (B, c.numEqsX)), self._t(sZ, "sZ", u8, (B, c.numEqsZ)),
                                      ctypes.c_void_p(self._stream(stream))), "qec_syndrome_dev")

    def statistics_dev(self, x, z, eX, eZ, flags, counters, stream=None):
        """Adds the batch's CodeStatistics counters into the int64 device tensor counters[8]
        (order: MC_COUNTERS)."""
        import torch
        self._single("statistics_dev")
        c = self.code
        B = x.shape[0]
        u8 = torch.uint8
        _check(lib().qec_statistics_dev(self._h, self._t(x, "x", u8, (B, c.n)), self._t(z, "z", u8, (B, c.n)),
                                        self._t(eX, "eX", u8, (B, c.n)), self._t(eZ, "eZ", u8, (B, c.n)),
                                        self._t(flags, "flags", u8, (B,)), B,
                                        self._t(counters, "counters", torch.int64, (len(MC_COUNTERS),)),
                                        ctypes.c_void_p(self._stream(stream))), "qec_statistics_dev")

    def statistics_packed_dev(self, errp, records, counters, iters=None, stream=None):
        """Adds the counters of packed errors + packed decision records into counters (int64 device
        tensor: [8] = MC_COUNTERS, or [10] = MC_COUNTERS_ALL when iters [B, 2] is given)."""
        import torch
        self._single("statistics_packed_dev")
        c = self.code
        B = errp.shape[0]
        nc = len(MC_COUNTERS_ALL) if iters is not None else len(MC_COUNTERS)
        _check(lib().qec_statistics_packed_dev(self._h, self._t(errp, "errp", torch.uint8, (B, 2 * ((c.n + 7) // 8))),
                                               self._t(records, "records", torch.uint8, (B, self.record_bytes())),
                                               self._t(iters, "iters", torch.int32, (B, 2), True), B,
                                               self._t(counters, "counters", torch.int64, (nc,)),
                                               ctypes.c_void_p(self._stream(stream))), "qec_statistics_packed_dev")

    def logical_packed_dev(self, errp, records, outcome, stream=None):
        """Per-sample outcome of packed errors + packed decision records into outcome [B] (uint8 device
        tensor): OUTCOME_SYNDROME_FAIL if the record flags a syndrome failure, else OUTCOME_LOGICAL if
        the residual fails the code's logical check, else OUTCOME_CORRECTED."""
        import torch
        self._single("logical_packed_dev")
        c = self.code
        B = errp.shape[0]
        _check(lib().qec_logical_packed_dev(self._h, self._t(errp, "errp", torch.uint8, (B, 2 * ((c.n + 7) // 8))),
                                            self._t(records, "records", torch.uint8, (B, self.record_bytes())),
                                            B, self._t(outcome, "outcome", torch.uint8, (B,)),
                                            ctypes.c_void_p(self._stream(stream))), "qec_logical_packed_dev")

    def pack_decisions_dev(self, eX, eZ, flags, out, stream=None):
        """Bit-packs a decoded device batch into out [B, record_bytes()] (uint8 device tensor)."""
        import torch
        self._single("pack_decisions_dev")
        c = self.code
        B = eX.shape[0]
        u8 = torch.uint8
        _check(lib().qec_pack_decisions_dev(self._h, self._t(eX, "eX", u8, (B, c.n)), self._t(eZ, "eZ", u8, (B, c.n)),
                                            self._t(flags, "flags", u8, (B,)), B,
                                            self._t(out, "out", u8, (B, self.record_bytes())),
                                            ctypes.c_void_p(self._stream(stream))), "qec_pack_decisions_dev")

    # ---- Monte-Carlo ---------------------------------------------------------------------
    def monte_carlo(self, seed, start, count, p, max_iter, stop="syndrome", batch=1 << 20):
        """Device Monte-Carlo run (sample -> syndrome -> decode -> statistics); returns a dict.  With priors
        set: sample_independent_dev's errors decoded with the priors, p not used."""
        r = MCResult()
        _check(lib().qec_monte_carlo(self._h, seed & (2 ** 64 - 1), start, count, float(p), int(max_iter),
                                     STOP[stop], batch, ctypes.byref(r)), "qec_monte_carlo")
        return r.as_dict()

    def Decode(self, syndromeX, syndromeZ, errorProbability, maxIterations):
        """Decoder::Decode for one syndrome pair -> (ErrorCode, outErrorsX, outErrorsZ)."""
        eX, eZ, flags, _, _ = self.decode_batch(syndrome_bytes(syndromeX)[None], syndrome_bytes(syndromeZ)[None],
                                                errorProbability, maxIterations, "ref")
        return int(flags[0]), eX[0].astype(np.int32), eZ[0].astype(np.int32)

    def GetStatistics(self, errorWeight, numErrors, errorProbability, maxIterations, seed=None, nThreads=1):
        if seed is None:
            seed = int.from_bytes(os.urandom(4), "little")
        st = Stats()
        _check(lib().qec_get_statistics(self._h, errorWeight, numErrors, float(errorProbability), maxIterations,
                                        seed & 0xFFFFFFFF, nThreads, ctypes.byref(st)), "qec_get_statistics")
        return st.as_dict()


class DecoderCPU(DecoderGPU):
    """The reference's DecoderCPU slot (QEC_LDPC/DecoderCPU.h): the library's CPU engine
    (device -1; host threads, bit-identical decisions).  Host-buffer entry points and
    GetStatistics only."""

    def __init__(self, code):
        super().__init__(code, device=-1, engine="cpu")

    def GetStatistics(self, errorWeight, numErrors, errorProbability, maxIterations, seed=None, nThreads=None):
        # the reference tests (numErrors / threads) * threads samples with its OpenMP thread count
        return super().GetStatistics(errorWeight, numErrors, errorProbability, maxIterations, seed,
                                     nThreads if nThreads is not None else 1)


def format_statistics(code, st):
    """CodeStatistics operator<< text block (QEC_LDPC/CodeStatistics.h:22-37)."""
    return ("Code: %s\nRand Seed: %d\nDuration(micro-s): %d\nErrors Tested: %d\nErrors With X: %d\n"
            "Errors With Z: %d\nError Weight: %d\nCorrected: %d\nSyndrome Errors X: %d\n"
            "Syndrome Errors Z: %d\nLogical Errors: %d\nConvergence Fail X: %d\nConvergence Fail Z: %d\n"
            % (code.describe(), st["randSeed"], st["durationMicroSeconds"], st["numErrorsTested"],
               st["numXErrorsTested"], st["numZErrorsTested"], st["errorWeight"], st["corrected"],
               st["syndromeErrorsX"], st["syndromeErrorsZ"], st["logicalErrors"], st["convergenceFailX"],
               st["convergenceFailZ"]))
