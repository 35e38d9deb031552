"""device_mem.h (DevBuf, DevArena) on the host: tests/device_mem_check.cpp supplies hipMalloc / hipFree itself, is built
with AddressSanitizer and UBSan and run as a child process.  No GPU, no HIP runtime, nothing loaded into Python."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CLANG = Path("/opt/rocm/llvm/bin/clang++")
ROCM_INCLUDE = Path("/opt/rocm/include")


def test_device_mem_header_sanitized(tmp_path):
    if not CLANG.exists() or not (ROCM_INCLUDE / "hip" / "hip_runtime_api.h").exists():
        pytest.skip(f"{CLANG} or the HIP headers under {ROCM_INCLUDE} are not installed")
    exe = tmp_path / "device_mem_check"
    build = subprocess.run(
        [str(CLANG), "-std=c++17", "-D__HIP_PLATFORM_AMD__", f"-I{ROCM_INCLUDE}", f"-I{ROOT / 'helicon_amd' / 'csrc'}",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1", "-Wall", "-Wextra", "-Werror",
         "-Wno-self-move", str(ROOT / "tests" / "device_mem_check.cpp"), "-o", str(exe)],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "device_mem_check: ok (live 0)" in run.stdout, run.stdout + run.stderr


@pytest.mark.parametrize("misuse", [
    "DevBuf<int> b = a;",                        # a copy
    "b = a;",                                    # a copy assignment
    "std::printf(\"%p\", a);",                   # a C variadic argument list
    "take_all(a);",                              # a by-value template parameter pack, as a launch wrapper has
])
def test_device_buffer_misuse_does_not_compile(tmp_path, misuse):
    """A DevBuf handed to a launch's argument list by value must be a compile error, not a copy in the kernel arguments."""
    if not CLANG.exists() or not (ROCM_INCLUDE / "hip" / "hip_runtime_api.h").exists():
        pytest.skip(f"{CLANG} or the HIP headers under {ROCM_INCLUDE} are not installed")
    body = "DevBuf<int> b; (void)b;" if misuse.startswith(("b =", "std::", "take")) else ""
    src = tmp_path / "misuse.cpp"
    src.write_text('#include "device_mem.h"\n#include <cstdio>\ntemplate <class... A> void take_all(A...) {}\n'
                   "void f(DevBuf<int>& a) { %s %s }\n" % (body, misuse))
    cmd = [str(CLANG), "-std=c++17", "-D__HIP_PLATFORM_AMD__", f"-I{ROCM_INCLUDE}", f"-I{ROOT / 'helicon_amd' / 'csrc'}",
           "-fsyntax-only", str(src)]
    assert subprocess.run(cmd, capture_output=True, text=True).returncode != 0, misuse
    src.write_text(src.read_text().replace(misuse, "int* p = a; (void)p;"))   # the same file without the misuse compiles
    ok = subprocess.run(cmd, capture_output=True, text=True)
    assert ok.returncode == 0, ok.stderr
