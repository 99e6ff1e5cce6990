"""bench.py --dump-outputs: the arrays the last timed step produced, written as float32 .npy files (a fixed
seeded sample of rows where all of them would be too many), and what a plain run's JSON line holds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import bench  # noqa: E402


def test_dump_outputs_rows_and_sample(tmp_path, monkeypatch):
    import torch
    rec = torch.arange(1000 * 7, dtype=torch.int64).remainder(251).to(torch.uint8).reshape(1000, 7)
    its = torch.arange(2000, dtype=torch.int32).reshape(1000, 2)
    bench.dump_outputs(str(tmp_path / "all"), ("records", "iters"), (rec, its), 0, 1)
    r = np.load(tmp_path / "all" / "records.npy")
    assert r.dtype == np.float32 and np.array_equal(r, rec.numpy())
    assert np.array_equal(np.load(tmp_path / "all" / "iters.npy"), its.numpy())
    assert np.array_equal(np.load(tmp_path / "all" / "rows.npy"), np.arange(1000))
    # 9 elements per row: 100 rows fit in 3600 bytes of float32; the same rows at every call
    monkeypatch.setattr(bench, "DUMP_BYTES", 3600)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), ("records", "iters"), (rec, its), 0, 1)
    rows = np.load(tmp_path / "a" / "rows.npy")
    assert rows.dtype == np.float64 and len(rows) == 100 and np.all(np.diff(rows) > 0) and rows[-1] < 1000
    assert np.array_equal(rows, np.load(tmp_path / "b" / "rows.npy"))
    idx = rows.astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "records.npy"), rec.numpy()[idx])
    assert np.array_equal(np.load(tmp_path / "a" / "iters.npy"), its.numpy()[idx])
    # a rank of several writes its own files
    bench.dump_outputs(str(tmp_path / "a"), ("records", "iters"), (rec, its), 1, 2)
    assert np.array_equal(np.load(tmp_path / "a" / "records_rank1.npy"), rec.numpy()[idx])


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step(tmp_path, code_paths):
    """A plain run times exactly --steps steps, measures nothing else, and its dumped records and iteration
    counts are those of the same call made here on the same seeded syndromes."""
    import torch

    import qec_ldpc_amd as q
    from qec_ldpc_amd.synthetic import bit_rows
    B = 4096 + 37
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--global-batch",
                        str(B), "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, "rc=%d\n%s\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, lines
    b = lines[0]
    assert b["steps"] == 2 and b["warmup"] == 1 and b["ms_per_step"] > 0 and b["unit"] == "syndromes/s"
    # ms_per_step is the time of one of the steps behind `value` (printed to 1e-4 ms)
    assert abs(B / b["value"] * 1e3 - b["ms_per_step"]) <= 1e-4 + 1e-6 * b["ms_per_step"]
    for key in ("full_arithmetic", "other_input", "ref_stop", "sustained", "graph", "cpu_baseline", "published_blocks",
                "sector_iterations", "gather"):
        assert key not in b, key

    code = q.Quantum_LDPC_Code.createFromFile(code_paths["P61"])
    dev = torch.device("cuda", 0)
    dec = q.DecoderGPU(code, 0, max_batch=B)
    sX = torch.empty((B, code.numEqsX), dtype=torch.uint8, device=dev)
    sZ = torch.empty((B, code.numEqsZ), dtype=torch.uint8, device=dev)
    dec.sample_syndrome_dev(bench.SEED, 0, 0.01, sX, sZ)
    rec = torch.empty((B, dec.record_bytes()), dtype=torch.uint8, device=dev)
    its = torch.empty((B, 2), dtype=torch.int32, device=dev)
    dec.decode_bits_packed_dev(bit_rows(sX), bit_rows(sZ), 0.01, 50, "fixed", rec, its)
    torch.cuda.synchronize()
    got = {n: np.load(os.path.join(str(tmp_path), n + ".npy")) for n in ("records", "iters", "rows")}
    assert got["records"].dtype == np.float32 and got["iters"].dtype == np.float32
    assert np.array_equal(got["rows"], np.arange(B))
    assert np.array_equal(got["records"], rec.cpu().numpy())
    assert np.array_equal(got["iters"], its.cpu().numpy())
