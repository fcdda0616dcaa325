"""examples/monet/train.py runs end to end on the GPU at a small size, in a fresh process, fp32 and bf16: the loss falls, and the model
that reads the pseudo-coordinates beats its own control, the same model with every edge's coordinates held constant."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_monet_example(cuda_device, bf16):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "monet", "train.py"), "--synthetic", "--nodes", "2000",
                          "--degree", "6", "--hidden", "32", "--epochs", "31"] + (["--bf16"] if bf16 else []),
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    loss = [float(v) for v in re.findall(r"loss ([0-9.]+)", res.stdout)]
    real, held = (float(v) for v in re.search(r"pseudo-coordinates ([0-9.]+), with them held constant ([0-9.]+)", res.stdout).groups())
    print(res.stdout)
    assert len(loss) == 4 and loss[-1] < loss[0], res.stdout
    assert 0.0 <= held <= 1.0 and real > held + 0.2, res.stdout
