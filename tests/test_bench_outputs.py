"""bench.py's plain run and --dump-outputs on the GPU: the line carries the headline fields and none of the
side measurements of --full, --steps sets the number of timed steps, and the dumped coefficients are the
oracle's transform of the bench's seeded images, bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *argv, "--timeout", "240"],
                         env=env, capture_output=True, text=True, timeout=300)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert out.returncode == 0 and lines, (out.returncode, out.stdout[-1500:], out.stderr[-3000:])
    return json.loads(lines[-1])


def test_plain_run_dumps_the_last_steps_coefficients(oracle, tmp_path):
    n, J, nb = 1024, 3, 2
    line = run_bench("--size", str(n), "--levels", str(J), "--images", str(nb), "--steps", "3", "--warmup", "1",
                     "--placements", "1", "--dump-outputs", str(tmp_path))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["step_ms_rank0"]["n"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
    for k in ("first_placement", "value_first_placement", "shard_sweep", "single_image", "batch_inverse", "host_pointer", "cpu_baseline"):
        assert k not in line, k  # side measurements belong to --full
    assert sorted(os.listdir(tmp_path)) == ["coefficients.npy"]
    got = np.load(tmp_path / "coefficients.npy")
    assert got.dtype == np.float32 and got.shape == (nb, n, n)

    import torch

    gen = torch.Generator(device="cuda")
    img = torch.empty((n, n), device="cuda", dtype=torch.float32)
    for k in range(nb):  # bench.py's seeded_images: image k seeded 1234 + k, generated on the device
        gen.manual_seed(1234 + k)
        torch.rand((n, n), generator=gen, out=img)
        want = img.cpu().numpy()
        assert oracle.fwd("cdf97_2f_s", want, J) == J
        assert np.array_equal(bits(got[k]), bits(want)), k
