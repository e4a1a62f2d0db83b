"""The graphs share one step() entry: a caller on another stream is ordered onto the graph's main stream and back, a caller already
on the main stream runs the step directly.  Both paths give the same bits (tests/_step_entry_child.py, under EVC_DETERMINISTIC=1,
which a process reads once: hence the child).  pytest -m gpu."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_step_gives_the_same_bits_from_the_default_stream_and_from_the_main_stream():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(root, "tests", "_step_entry_child.py")],
                       env=dict(os.environ, EVC_DETERMINISTIC="1"), capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith("ok")
