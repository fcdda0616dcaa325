"""examples/deepergcn/train.py runs end to end on the GPU at a small size, in a fresh process, fp32 and bf16: the loss falls over a few
epochs, the closing lines parse, and the learned t has left its initial value."""
import os
import re
import subprocess
import sys

import pytest

from dgll_amd.nn.Convolution import GENConv  # noqa: F401  (what the example trains)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_deepergcn_example(cuda_device, bf16):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "deepergcn", "train.py"), "--synthetic", "--nodes", "2000",
                          "--hidden", "32", "--epochs", "8"] + (["--bf16"] if bf16 else []),
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    loss = [float(v) for v in re.findall(r"loss ([0-9.]+)", res.stdout)]
    acc = [float(v) for v in re.search(r"learned t ([0-9.]+), with t frozen at 0 \(the mean\) ([0-9.]+)", res.stdout).groups()]
    start, values = re.search(r"learned t per layer, from ([0-9.-]+): (.*)", res.stdout).groups()
    assert len(loss) == 8 and loss[-1] < loss[0], res.stdout
    assert all(0.0 <= v <= 1.0 for v in acc), res.stdout
    learned = [float(v) for v in values.split()]
    assert len(learned) == 3 and all(v != float(start) for v in learned), res.stdout
