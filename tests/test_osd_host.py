"""BP + OSD-0 post-processing (QEC_OPT_OSD) without a GPU: the host
implementation (osd_host.cpp) through qec_osd and the CPU engine's synchronous calls, the options,
and the CLI, against a numpy restatement of the definition (dense uint8 elimination) whose soft input
and BP outputs come from the oracle.  tests/test_gpu_osd.py reuses the yardstick for the kernel."""
import os
import re
import subprocess

import numpy as np
import pytest

import qec_ldpc_amd as q
from conftest import ROOT
from oracle.oracle import OracleCode
from qec_ldpc_amd.codes import write_code_file
from qec_ldpc_amd.gather import pack_records
from qec_ldpc_amd.synthetic import depolarizing_errors

CLI = os.path.join(ROOT, "tools", "qec_ldpc")
G13 = (3, 3, 6, 13, 3, 2)  # n = 78: the bit-packed rows cross a 64-bit boundary
KEYS = ["P7", "G13", "P61"]
# p, iteration cap of the main decode (syndrome stop), batch, failed samples it must leave at least
MAIN = {"P7": (0.05, 20, 600, 100), "G13": (0.05, 25, 600, 30), "P61": (0.06, 50, 192, 15)}
FAIL = (q.SYNDROME_FAIL_X, q.SYNDROME_FAIL_Z)


# ---- the yardstick: section 1.2 in numpy -------------------------------------------------------
def gf2_rank(H):
    A = H.copy().astype(np.uint8)
    r = 0
    for v in range(A.shape[1]):
        rows = np.nonzero(A[r:, v])[0]
        if not len(rows):
            continue
        p = r + rows[0]
        A[[r, p]] = A[[p, r]]
        below = np.nonzero(A[r + 1:, v])[0] + r + 1
        A[below] ^= A[r]
        r += 1
        if r == A.shape[0]:
            break
    return r


def osd_keys(r):
    """Step 2: NaN -> the pattern of 0.5f, else the pattern with the sign bit cleared."""
    a = np.ascontiguousarray(r, dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)
    return np.where(a > 0x7F800000, np.uint32(0x3F000000), a).astype(np.uint32)


class Yardstick:
    """One code: its matrices, their ranks, and for each sector the q_final offset of the message at
    the lowest-index check that contains v (layout [check][slot], slots in ascending variable order,
    X block first)."""

    def __init__(self, code):
        self.n, self.L = code.n, code.L
        self.H = [code.pcm(0), code.pcm(1)]
        self.rank = [gf2_rank(h) for h in self.H]
        self.qn = (code.numEqsX + code.numEqsZ) * code.L
        self.pos = []
        base = 0
        for H in self.H:
            pos = np.empty(self.n, dtype=np.int64)
            for v in range(self.n):
                c = int(np.nonzero(H[:, v])[0][0])
                pos[v] = base + c * self.L + int(H[c, :v].sum())
            self.pos.append(pos)
            base += H.shape[0] * self.L

    def sector(self, sec, s, qrow):
        """Steps 2-6 for one sector: the new estimate, or None if [H | s] is inconsistent."""
        H, n = self.H[sec], self.n
        key = osd_keys(qrow[self.pos[sec]]).astype(np.int64)
        order = np.lexsort((np.arange(n), -key))  # key descending, ties by v ascending
        A = np.concatenate([H, np.asarray(s, dtype=np.uint8)[:, None] & 1], axis=1).astype(np.uint8)
        used = np.zeros(H.shape[0], dtype=bool)
        piv = []
        for v in order:
            if len(piv) == self.rank[sec]:
                break
            rows = np.nonzero(A[:, v].astype(bool) & ~used)[0]
            if not len(rows):
                continue  # dependent on the pivots chosen so far
            p = rows[0]
            others = A[:, v].astype(bool)
            others[p] = False
            A[others] ^= A[p]
            used[p] = True
            piv.append((p, v))
        if A[~used, n].any():
            return None
        e = np.zeros(n, dtype=np.uint8)
        for p, v in piv:
            e[v] = A[p, n]
        return e

    def repair(self, sX, sZ, qf, eX, eZ, flags):
        """Steps 2-7 on a decoded batch -> repaired copies and the number of sectors repaired."""
        eX, eZ, flags = eX.copy(), eZ.copy(), flags.copy()
        count = 0
        for b in range(len(flags)):
            for sec, (s, e) in enumerate(((sX, eX), (sZ, eZ))):
                if not flags[b] & FAIL[sec]:
                    continue
                new = self.sector(sec, s[b], qf[b])
                if new is not None:
                    e[b] = new
                    flags[b] &= ~FAIL[sec] & 0xFF
                    count += 1
        return eX, eZ, flags, count

    def bp_osd(self, orc, sX, sZ, p, N, stop, n_osd=3):
        """The whole of section 1.2: the oracle's main decode, its fixed-stop soft decode of the
        failed samples, the repair.  -> (eX, eZ, flags, iters, sectors repaired, main decode's flags)."""
        eX, eZ, flags, iters = orc.decode_batch(sX, sZ, p, N, stop)[:4]
        bad = np.nonzero(flags & 3)[0]
        out = (eX, eZ, flags, 0)
        if len(bad):
            qf = orc.decode_batch(sX[bad], sZ[bad], p, n_osd, "fixed", want_q=True)[4].reshape(len(bad), self.qn)
            rX, rZ, rf, cnt = self.repair(sX[bad], sZ[bad], qf, eX[bad], eZ[bad], flags[bad])
            oX, oZ, of = eX.copy(), eZ.copy(), flags.copy()
            oX[bad], oZ[bad], of[bad] = rX, rZ, rf
            out = (oX, oZ, of, cnt)
        return out + (iters, flags)


def random_soft(rng, B, qn):
    """Soft input with exact ties, 0, 1, NaN of both signs, -0.0 and negative values."""
    qf = rng.random((B, qn), dtype=np.float32)
    qf = np.where(rng.random((B, qn)) < 0.5, np.round(qf * 8) / 8, qf).astype(np.float32)  # ties, 0 and 1
    qf = np.where(rng.random((B, qn)) < 0.2, -qf, qf).astype(np.float32)                    # signs, -0.0
    bits = qf.view(np.uint32).copy()
    r = rng.random((B, qn))
    bits[r < 0.03] = 0x7FC00000
    bits[(r >= 0.03) & (r < 0.06)] = 0xFFC00001
    bits[(r >= 0.06) & (r < 0.08)] = 0x80000000
    bits[(r >= 0.08) & (r < 0.10)] = 0x3F800000
    return bits.view(np.float32)


def forced_batch(code, rng, B):
    """A decoded batch in which every sector is marked failed: sampled (consistent) syndromes, junk
    estimates, random convergence bits, random soft input."""
    x, z = depolarizing_errors(code.n, 31337, B, 0.08)
    sX, sZ = code.syndrome(0, x), code.syndrome(1, z)
    eX = rng.integers(0, 2, (B, code.n), dtype=np.uint8)
    eZ = rng.integers(0, 2, (B, code.n), dtype=np.uint8)
    flags = (3 | (rng.integers(0, 4, B) << 2)).astype(np.uint8)
    qf = random_soft(rng, B, (code.numEqsX + code.numEqsZ) * code.L)
    return sX, sZ, qf, eX, eZ, flags


def make_codes(code_paths, tmp):
    """key -> (code, path of a code file the oracle loads)."""
    out = {}
    for k in ("P7", "P61"):
        out[k] = (q.Quantum_LDPC_Code.createFromFile(code_paths[k]), code_paths[k])
    g = q.QC_LDPC_CSS(*G13).with_logical("degenerate")
    path = write_code_file(str(tmp / "g13_degenerate.txt"), g.J, g.K, g.L, g.P, g.sigma, g.tau, g.pcm(0), g.pcm(1),
                           IMP=g.imp())
    out["G13"] = (g, path)
    return out


_main_cache = {}


def main_case(env, key):
    """The sampled batch of MAIN[key] and the yardstick's BP + OSD result for it (computed once)."""
    if key not in _main_cache:
        code, _, orc, ys = env[key]
        p, N, B, _ = MAIN[key]
        x, z = depolarizing_errors(code.n, 5000, B, p)
        sX, sZ = code.syndrome(0, x), code.syndrome(1, z)
        _main_cache[key] = (sX, sZ, x, z, ys.bp_osd(orc, sX, sZ, p, N, "syndrome"))
    return _main_cache[key]


def check_main_conditions(code, key, sX, sZ, want):
    """Conditions, not measurements: enough failures before, none after, H e = s everywhere."""
    eX, eZ, flags, cnt, _, flags0 = want
    assert int(((flags0 & 3) != 0).sum()) >= MAIN[key][3]
    assert not (flags & 3).any()
    assert np.array_equal(code.syndrome(0, eX), sX) and np.array_equal(code.syndrome(1, eZ), sZ)
    assert cnt == int(np.unpackbits((flags0 & 3)[:, None], axis=1).sum())


@pytest.fixture(scope="module")
def env(code_paths, tmp_path_factory):
    out = {}
    for k, (code, path) in make_codes(code_paths, tmp_path_factory.mktemp("osd_codes")).items():
        out[k] = (code, q.DecoderCPU(code), OracleCode(path), Yardstick(code))
    return out


# ---- tests ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_qec_osd_matches_numpy_on_random_soft_input(env, key):
    code, dec, _, ys = env[key]
    B = 8 if key == "P61" else 32
    sX, sZ, qf, eX, eZ, flags = forced_batch(code, np.random.default_rng(11), B)
    wX, wZ, wf, cnt = ys.repair(sX, sZ, qf, eX, eZ, flags)
    assert cnt == 2 * B and not (wf & 3).any() and np.array_equal(wf & 12, flags & 12)
    gX, gZ, gf = dec.osd(sX, sZ, qf, eX, eZ, flags)
    assert np.array_equal(gX, wX) and np.array_equal(gZ, wZ) and np.array_equal(gf, wf)
    assert dec.get_option("osd_sectors") == cnt
    # a sector without its fail bit is left alone
    part = flags.copy()
    part[::2] &= ~1 & 0xFF
    part[1::3] &= ~2 & 0xFF
    gX, gZ, gf = dec.osd(sX, sZ, qf, eX, eZ, part)
    keepX, keepZ = (part & 1) == 0, (part & 2) == 0
    assert np.array_equal(gX[keepX], eX[keepX]) and np.array_equal(gZ[keepZ], eZ[keepZ])
    assert np.array_equal(gX[~keepX], wX[~keepX]) and np.array_equal(gZ[~keepZ], wZ[~keepZ])
    assert np.array_equal(gf, part & 12)


def inconsistent_syndrome(ys, sec, s, rng):
    """Flip bits of a sampled syndrome until the yardstick finds [H | s] inconsistent."""
    s = s.copy()
    q0 = np.zeros(ys.qn, dtype=np.float32)
    for _ in range(64):
        if ys.sector(sec, s, q0) is None:
            return s
        s[rng.integers(0, len(s))] ^= 1
    raise AssertionError("no inconsistent syndrome found")


@pytest.mark.parametrize("key", KEYS)
def test_inconsistent_syndrome_is_left_alone(env, key):
    code, dec, _, ys = env[key]
    rng = np.random.default_rng(5)
    sX, sZ, qf, eX, eZ, flags = forced_batch(code, rng, 4)
    deficient = [sec for sec in (0, 1) if ys.rank[sec] < ys.H[sec].shape[0]]
    assert deficient, "every shipped matrix is rank deficient"
    for sec in deficient:
        s = (sX, sZ)[sec]
        s[1] = inconsistent_syndrome(ys, sec, s[1], rng)
    wX, wZ, wf, cnt = ys.repair(sX, sZ, qf, eX, eZ, flags)
    assert cnt == 8 - len(deficient)
    gX, gZ, gf = dec.osd(sX, sZ, qf, eX, eZ, flags)
    assert np.array_equal(gX, wX) and np.array_equal(gZ, wZ) and np.array_equal(gf, wf)
    for sec in deficient:  # estimate and flag as BP left them
        assert gf[1] & FAIL[sec]
        assert np.array_equal((gX, gZ)[sec][1], (eX, eZ)[sec][1])
    assert dec.get_option("osd_sectors") == cnt


@pytest.mark.parametrize("key", KEYS)
def test_decoder_cpu_with_osd(env, key):
    code, dec, _, _ = env[key]
    p, N, B, _ = MAIN[key]
    sX, sZ, _, _, want = main_case(env, key)
    check_main_conditions(code, key, sX, sZ, want)
    eX, eZ, flags, cnt, iters, flags0 = want
    # option off: today's outputs
    off = dec.decode_batch(sX, sZ, p, N, "syndrome", want_iters=True)
    assert np.array_equal(off[2], flags0) and np.array_equal(off[3], iters)
    assert dec.get_option("osd_sectors") == 0 and dec.last_path() == set()
    rec_off, _ = dec.decode_batch_packed(sX, sZ, p, N, "syndrome")
    assert np.array_equal(rec_off, pack_records(off[0], off[1], off[2]))
    dec.set_option("osd", 1)
    try:
        assert dec.get_option("osd") == 1 and dec.get_option("osd_iterations") == 3
        g = dec.decode_batch(sX, sZ, p, N, "syndrome", want_iters=True)
        assert np.array_equal(g[0], eX) and np.array_equal(g[1], eZ) and np.array_equal(g[2], flags)
        assert np.array_equal(g[3], iters)  # still the main decode's iterations
        assert dec.get_option("osd_sectors") == cnt and dec.last_path() == {"osd"}
        rec, its = dec.decode_batch_packed(sX, sZ, p, N, "syndrome", want_iters=True)
        assert np.array_equal(rec, pack_records(eX, eZ, flags)) and np.array_equal(its, iters)
        assert dec.get_option("osd_sectors") == cnt
    finally:
        dec.set_option("osd", 0)
    again = dec.decode_batch(sX, sZ, p, N, "syndrome")
    assert all(np.array_equal(a, b) for a, b in zip(again[:3], off[:3]))
    assert dec.get_option("osd_sectors") == 0


def test_osd_iterations_feed_the_order(env):
    """Another iteration count is another soft input: the library follows the yardstick there too."""
    code, dec, orc, ys = env["G13"]
    p, N, B, _ = MAIN["G13"]
    sX, sZ = main_case(env, "G13")[:2]
    want = ys.bp_osd(orc, sX, sZ, p, N, "syndrome", n_osd=1)
    dec.set_option("osd", 1)
    dec.set_option("osd_iterations", 1)
    try:
        g = dec.decode_batch(sX, sZ, p, N, "syndrome")
    finally:
        dec.set_option("osd_iterations", 3)
        dec.set_option("osd", 0)
    assert np.array_equal(g[0], want[0]) and np.array_equal(g[1], want[1]) and np.array_equal(g[2], want[2])


def test_get_statistics_with_osd(env):
    """GetStatistics on the CPU engine, option on: host counting over the numpy-repaired estimates."""
    code, dec, orc, ys = env["P7"]
    W, count, p, N, seed = 6, 1500, 0.05, 20, 20240607
    x, z = q.sample_fixed_weight(seed, W, count, code.n)
    sX, sZ = code.syndrome(0, x), code.syndrome(1, z)
    eX, eZ, flags, cnt, _, flags0 = ys.bp_osd(orc, sX, sZ, p, N, "ref")
    assert int(((flags0 & 3) != 0).sum()) >= 50 and not (flags & 3).any()
    logical = code.check_logical(x ^ eX, z ^ eZ)
    want = {"numErrorsTested": count, "numXErrorsTested": int(x.any(1).sum()), "numZErrorsTested": int(z.any(1).sum()),
            "corrected": int((~logical).sum()), "logicalErrors": int(logical.sum()), "syndromeErrorsX": 0,
            "syndromeErrorsZ": 0, "convergenceFailX": int(((flags & 4) != 0).sum()),
            "convergenceFailZ": int(((flags & 8) != 0).sum())}
    dec.set_option("osd", 1)
    try:
        st = dec.GetStatistics(W, count, p, N, seed)
        assert dec.get_option("osd_sectors") == cnt
    finally:
        dec.set_option("osd", 0)
    assert {k: st[k] for k in want} == want
    off = dec.GetStatistics(W, count, p, N, seed)
    assert off["syndromeErrorsX"] == int(((flags0 & 1) != 0).sum())
    assert off["syndromeErrorsZ"] == int(((flags0 & 2) != 0).sum())
    assert dec.get_option("osd_sectors") == 0


def test_option_and_argument_checks(env):
    code, dec, _, _ = env["P7"]
    assert dec.get_option("osd") == 0 and dec.get_option("osd_iterations") == 3 and dec.get_option("osd_sectors") == 0
    for name, value in (("osd", 2), ("osd", -1), ("osd_iterations", 0), ("osd_sectors", 0), ("osd_sectors", 5),
                        ("osd_sweep", 3)):
        with pytest.raises(q.QecError):
            dec.set_option(name, value)
    assert dec.get_option("osd") == 0 and dec.get_option("osd_iterations") == 3
    dec.set_option("osd_iterations", 7)
    assert dec.get_option("osd_iterations") == 7
    dec.set_option("osd_iterations", 3)
    assert q.PATH["osd"] == 256 and {"qec_osd", "qec_osd_dev"} <= set(q.EXPORTS)
    rc = q.lib().qec_osd(dec._h, None, None, 1, None, None, None, None)
    assert rc == -1 and "qec_osd" in q.last_error()
    one = np.zeros(8, dtype=np.uint8)  # the CPU engine has no device buffers: refused before any is read
    ptr = one.ctypes.data_as(q.ctypes.c_void_p)
    assert q.lib().qec_osd_dev(dec._h, ptr, ptr, 1, ptr, ptr, ptr, ptr, None) == -4


def _cli(tmp_path, flags, code, line):
    (tmp_path / "results").mkdir(exist_ok=True)
    (tmp_path / "init.txt").write_text("%s %s\n" % (code, line))
    return subprocess.run([CLI] + flags + ["init.txt"], cwd=tmp_path, capture_output=True, text=True, timeout=120)


def _fields(tmp_path):
    (f,) = os.listdir(tmp_path / "results")
    text = (tmp_path / "results" / f).read_text()
    return dict(re.findall(r"^([A-Za-z ()\-]+): (.*)$", text, flags=re.M))


def test_cli_osd(tmp_path, code_paths):
    line = "6 6 2000 20 0.05"
    a, b = tmp_path / "off", tmp_path / "on"
    a.mkdir()
    b.mkdir()
    r = _cli(a, ["--engine", "cpu", "--seed", "7"], code_paths["P7"], line)
    assert r.returncode == 0, r.stderr
    r = _cli(b, ["--engine", "cpu", "--seed", "7", "--osd", "0", "--osd-iterations", "3"], code_paths["P7"], line)
    assert r.returncode == 0, r.stderr
    off, on = _fields(a), _fields(b)
    assert int(off["Syndrome Errors X"]) + int(off["Syndrome Errors Z"]) > 0
    assert int(on["Syndrome Errors X"]) == 0 and int(on["Syndrome Errors Z"]) == 0
    assert on["Errors Tested"] == off["Errors Tested"]
    assert int(on["Corrected"]) + int(on["Logical Errors"]) == int(on["Errors Tested"])
    for flags in (["--osd", "1"], ["--osd-iterations", "3"], ["--osd", "0", "--osd-iterations", "0"]):
        c = tmp_path / ("bad" + "_".join(flags).replace("-", ""))
        c.mkdir()
        r = _cli(c, ["--engine", "cpu"] + flags, code_paths["P7"], line)
        assert r.returncode == 2 and "usage: qec_ldpc" in r.stderr
