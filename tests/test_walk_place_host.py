"""twist_walk_place (sweep_plan.h: where the twist walk's workgroups stand in a launch) on the host:
tests/walk_place_check.cpp asserts the bijection, the even deal of the block-0 workgroups over the eight residue classes,
the contiguous eighths of the other blocks and the defect of the map it replaces (C2: all 240 in one class), is built with
AddressSanitizer and UBSan and run as a child process.  No GPU, no HIP runtime, nothing loaded into Python."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CLANG = Path("/opt/rocm/llvm/bin/clang++")


def test_walk_place_header_sanitized(tmp_path):
    if not CLANG.exists():
        pytest.skip(f"{CLANG} is not installed")
    exe = tmp_path / "walk_place_check"
    build = subprocess.run(
        [str(CLANG), "-std=c++17", f"-I{ROOT / 'helicon_amd' / 'csrc'}", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-g", "-O1", "-Wall", "-Wextra", "-Werror",
         str(ROOT / "tests" / "walk_place_check.cpp"), "-o", str(exe)],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "walk_place_check: ok" in run.stdout, run.stdout + run.stderr
