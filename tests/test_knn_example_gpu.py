"""examples/dgcnn/train.py runs end to end on the GPU at a small size, in a fresh process, fp32 and bf16: the loss falls over a few
epochs and the closing lines parse."""
import os
import re
import subprocess
import sys

import pytest

from dgll_amd.nn.Convolution import DGCNN  # noqa: F401  (what the example trains)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_dgcnn_example(cuda_device, bf16):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "dgcnn", "train.py"), "--synthetic", "--clouds", "60", "--points",
                          "96", "--k", "8", "--hidden", "16,16,32", "--emb", "64", "--epochs", "6", "--batch", "12"]
                         + (["--bf16"] if bf16 else []), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    loss = [float(v) for v in re.findall(r"loss ([0-9.]+)", res.stdout)]
    acc, count, chance = re.search(r"held-out accuracy ([0-9.]+) on (\d+) clouds \(chance ([0-9.]+)\)", res.stdout).groups()
    searches = int(re.search(r"(\d+) searches per step", res.stdout).group(1))
    assert len(loss) == 6 and loss[-1] < loss[0], res.stdout
    assert 0.0 <= float(acc) <= 1.0 and int(count) == 12 and abs(float(chance) - 1 / 6) < 1e-3 and searches == 3, res.stdout
