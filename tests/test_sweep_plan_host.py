"""sweep_plan.h (the host arithmetic of the two sweep drivers: launch caps, the cut of a list into table groups, batches and
pieces of a run, the ragged split, plan_runs, the general-size sweep's runs and layers) on the host:
tests/sweep_plan_check.cpp compares each function with a brute-force restatement or with properties on small random inputs,
is built with AddressSanitizer and UBSan and run as a child process.  No GPU, no HIP runtime, nothing loaded into Python."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CLANG = Path("/opt/rocm/llvm/bin/clang++")


def test_sweep_plan_header_sanitized(tmp_path):
    if not CLANG.exists():
        pytest.skip(f"{CLANG} is not installed")
    exe = tmp_path / "sweep_plan_check"
    build = subprocess.run(
        [str(CLANG), "-std=c++17", f"-I{ROOT / 'helicon_amd' / 'csrc'}", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-g", "-O1", "-Wall", "-Wextra", "-Werror",
         str(ROOT / "tests" / "sweep_plan_check.cpp"), "-o", str(exe)],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "sweep_plan_check: ok" in run.stdout, run.stdout + run.stderr
