"""python -m grapes_amd.full_batch end to end on the MI355X: Cora (the int32 autograd path) and papers100M (the row-blocked
64-bit path)."""
import gc
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, timeout):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    # the run needs ~150 GiB at papers100M: give back what this process's earlier tests left in torch's cache (and in reference
    # cycles of their tracebacks) before the child process starts
    gc.collect()
    torch.cuda.empty_cache()
    r = subprocess.run([sys.executable, "-m", "grapes_amd.full_batch"] + args, cwd=ROOT, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_cli_cora_runs_and_reports():
    out = _run(["--dataset", "cora", "--max_epochs", "10", "--eval_frequency", "5", "--runs", "2", "--seed", "0"], 600)
    assert out.count("valid_f1=") == 2 * 2 and out.count("test_f1=") == 2 and "Acc:" in out, out[-3000:]


def test_cli_papers100m_reaches_its_test_pass():
    out = _run(["--dataset", "papers100m", "--max_epochs", "1", "--runs", "1", "--seed", "0"], 1500)
    assert "test_f1=" in out and "Acc:" in out, out[-3000:]
