"""bench.py without --full: the headline run (set up, warm up, time --steps steps, print one JSON line)
and --dump-outputs (the last timed step's next-token ids as float64): two runs of the same command must
dump the same ids."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--layers", "2", "--bs", "8", "--seqlen", "256", "--steps", "3", "--warmup", "1"]


def _bench(out_dir):
    r = subprocess.run([sys.executable, "bench.py", *ARGS, "--dump-outputs", str(out_dir)], cwd=ROOT,
                       capture_output=True, text=True, timeout=560)
    assert r.returncode == 0, f"--- stdout\n{r.stdout[-3000:]}\n--- stderr\n{r.stderr[-3000:]}"
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, f"expected ONE JSON line, got {len(lines)}:\n{r.stdout[-2000:]}"
    return json.loads(lines[0])


@pytest.mark.timeout(1200)
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    recs = [_bench(tmp_path / "a"), _bench(tmp_path / "b")]
    for rec in recs:
        assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["ms_per_step"] > 0
        assert rec["unit"] == "tokens/s" and rec["higher_is_better"] is True and rec["dtype"].startswith("bf16")
        assert abs(rec["value"] - 8 * 1e3 / rec["ms_per_step"]) <= 0.01 * rec["value"]
        assert rec["roofline"] is None and rec["int4_gemm"] is None and rec["cpu_baseline"] is None
    a, b = (np.load(tmp_path / d / "next_tokens.npy") for d in ("a", "b"))
    assert a.dtype == np.float64 and a.shape == (8,)
    assert np.all(a == np.round(a)) and a.min() >= 0
    assert np.array_equal(a, b), f"two runs of the same command dumped different ids: {a} vs {b}"
