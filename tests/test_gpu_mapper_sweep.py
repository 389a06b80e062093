"""The randomised parity sweep of the depth mapper (tests/randomised/fuzz_mapper.py) at a size that fits the suite.  Longer runs:
``python tests/randomised/fuzz_mapper.py <cases> <seed>``."""

import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_randomised_sweep_of_the_mapper():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "randomised", "fuzz_mapper.py"), "6", "5"], capture_output=True, text=True,
                         timeout=600, cwd=ROOT)
    text = out.stdout + out.stderr
    print(text[-3000:])
    assert out.returncode == 0, text[-2000:]
    assert ", 0 failed" in text, text[-2000:]
