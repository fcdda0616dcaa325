"""examples/resgated/train.py runs end to end on the GPU at a small size, in a fresh process, fp32 and bf16: the loss falls over a few
epochs and the script reaches its closing accuracy line."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_resgated_example(cuda_device, bf16):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "resgated", "train.py"), "--synthetic", "--nodes", "2000",
                          "--degree", "6", "--hidden", "32", "--epochs", "8"] + (["--bf16"] if bf16 else []),
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    loss = [float(v) for v in re.findall(r"loss ([0-9.]+)", res.stdout)]
    acc = [float(v) for v in re.search(r"neighbours ([0-9.]+), with every edge removed ([0-9.]+)", res.stdout).groups()]
    assert len(loss) == 8 and loss[-1] < loss[0], res.stdout
    assert all(0.0 <= v <= 1.0 for v in acc), res.stdout
