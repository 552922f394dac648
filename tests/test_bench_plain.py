"""bench.py's plain run (the headline only), --full, and --dump-outputs.  The CPU tests run through the test engine
(tests.cpu_engine, oracle on the host); the GPU test checks the dumped bytes of the real engine against the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--streams", "64", "--stream-len", "4096"]


def _bench(args, test_engine=True, timeout=300):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    if test_engine:
        env["FLATE_BENCH_TEST_ENGINE"] = "tests.cpu_engine:OracleEngine"
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_plain_run_is_the_headline_and_dumps_the_same_outputs_every_time(tmp_path):
    runs = []
    for k in range(2):
        d = str(tmp_path / ("d%d" % k))
        line = _bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", d] + SMALL)
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
        assert line["unit"] == "GiB/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
        assert line["value"] > 0 and line["metric"].startswith("GiB/s")
        # nothing beyond the headline: no CPU leg, no parity check, no "extra"
        assert line["cpu_baseline"] is None and line["config"]["parity_checked_streams"] == 0 and "extra" not in line
        runs.append(_load(d))
    a, b = runs
    assert set(a) == {"offsets", "sample_bytes", "sample_streams"}
    assert a["sample_bytes"].dtype == np.float32 and a["offsets"].dtype == np.float64
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    # the sample is the concatenation of the chosen streams' compressed bytes
    off, idx = a["offsets"], a["sample_streams"].astype(np.int64)
    assert a["sample_bytes"].size == int(sum(off[i + 1] - off[i] for i in idx))
    assert a["offsets"].size == 65 and a["offsets"][-1] == line["config"]["compressed_bytes_per_gpu"]


def test_full_run_keeps_the_cpu_baseline_and_the_parity_check():
    line = _bench(["--full", "--gpus", "1", "--steps", "2", "--warmup", "1", "--cpu-sample-streams", "64"] + SMALL)
    assert line["steps"] == 2
    assert line["config"]["parity_checked_streams"] == 64 and line["cpu_baseline"]["value"] > 0


@pytest.mark.gpu
def test_dumped_streams_are_the_engines_bytes(tmp_path, oracle):
    """The plain run on the GPU: what --dump-outputs wrote is what the oracle produces for the sampled streams."""
    import importlib
    flate = importlib.import_module("moonbit-flate_amd")
    n, blen = 256, 65536
    d = str(tmp_path / "d")
    line = _bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--streams", str(n), "--dump-outputs", d],
                  test_engine=False, timeout=600)
    assert line["steps"] == 2 and line["cpu_baseline"] is None
    got = _load(d)
    off, idx, sample = got["offsets"].astype(np.int64), got["sample_streams"].astype(np.int64), got["sample_bytes"]
    assert off.size == n + 1 and int(off[-1]) == line["config"]["compressed_bytes_per_gpu"]
    data = flate.synth("text", n, blen)
    pos = 0
    for i in idx:
        ln = int(off[i + 1] - off[i])
        assert bytes(sample[pos:pos + ln].astype(np.uint8)) == oracle.deflate(data[i * blen:(i + 1) * blen]), i
        pos += ln
    assert pos == sample.size
