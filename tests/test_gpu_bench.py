"""bench.py on the device at a tiny size: a plain run prints the headline line alone, --steps sets the timed steps, and --dump-outputs writes the
last timed step's outputs, the same bytes from run to run (the inputs are seeded)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_plain_run_dumps_the_same_outputs_twice(gpu, tmp_path):
    lines = []
    for d in ("a", "b"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", "--width", "176", "--height", "144",
               "--streams", "8", "--distinct", "4", "--dump-outputs", str(tmp_path / d)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    for out in lines:
        assert out["steps"] == 4 and out["warmup"] == 2 and out["ms_per_step"] > 0 and out["value"] > 0
        assert (out["unit"], out["higher_is_better"], out["dtype"]) == ("frames/s", True, "u8")
        assert not {"roofline", "cpu_baseline", "e2e", "lookahead", "csp_ingest", "value_survey_content", "decoder_probe"} & set(out)
    n = ((176 + 15) // 16) * ((144 + 15) // 16)
    for name, width in (("mb_records", 64), ("levels", 416)):
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape == (8, n, width)
        assert np.array_equal(a, b), name
    # the timed steps code I P | I P Bref b: the last one is a b picture (B slice: B types and maybe intra, no P types), the warmup's last a P picture
    types = np.unique(np.load(tmp_path / "a" / "mb_records.npy")[:, :, 0]).astype(int)
    assert set(types) <= {0, 1, 2, 7, 8, 9, 10} and types.max() >= 7, types
