"""examples/gine/train_fused.py runs end to end on the GPU at a small size, in a fresh process, fp32 and bf16: the loss falls, the
model reads the edge attributes (accuracy with them well above the accuracy with them zeroed) and the script reaches its closing
line."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_fused_gine_example(cuda_device, bf16):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "gine", "train_fused.py"), "--synthetic", "--nodes", "2000",
                          "--degree", "8", "--hidden", "32", "--epochs", "31"] + (["--bf16"] if bf16 else []),
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    loss = [float(v) for v in re.findall(r"loss ([0-9.]+)", res.stdout)]
    real, zeroed = (float(v) for v in re.search(r"attributes ([0-9.]+), with them zeroed ([0-9.]+)", res.stdout).groups())
    assert len(loss) == 4 and loss[-1] < loss[0], res.stdout
    assert re.search(r"peak memory of a training step above the model and the data: [0-9.]+ MB", res.stdout), res.stdout
    assert real > zeroed + 0.2, res.stdout
