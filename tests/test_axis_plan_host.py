"""axis_plan.h (the host arithmetic of the separable axis passes: the geometry of a pass from its view or from a shape and an
axis, the operator-block builder, the unit circle) on the host: tests/axis_plan_check.cpp checks that every grid addresses
its input and output arrays exactly once and in row-major order, that the seven set-ups the header replaced give the same
offsets, and the builders against brute-force loops; it is built with AddressSanitizer and UBSan and run as a child process.
No GPU, no HIP runtime, nothing loaded into Python."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CLANG = Path("/opt/rocm/llvm/bin/clang++")


def test_axis_plan_header_sanitized(tmp_path):
    if not CLANG.exists():
        pytest.skip(f"{CLANG} is not installed")
    exe = tmp_path / "axis_plan_check"
    build = subprocess.run(
        [str(CLANG), "-std=c++17", f"-I{ROOT / 'helicon_amd' / 'csrc'}", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-g", "-O1", "-Wall", "-Wextra", "-Werror",
         str(ROOT / "tests" / "axis_plan_check.cpp"), "-o", str(exe)],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "axis_plan_check: ok" in run.stdout, run.stdout + run.stderr
