"""
The staged-output helper of the grouped pipelines (csrc/capi_staged_out.hpp) on the CPU: tests/staged_out_check.cpp is compiled with
the host compiler under the address and undefined-behaviour sanitizers and run.  It declares the grouped report's nine outputs,
the GLM set with and without its per-row outputs, outputs staged because the caller gave none on a device frame, slices of 0, 1
and 255 / 256 / 257 bytes and the rolling forms' two sets, and checks that every slice is 256-byte aligned, inside the block of
exactly bytes() bytes and apart from every other, and that an output which is not staged keeps the caller's pointer at no cost.
"""
import os
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_staged_outs_slices(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "staged_out_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(ROOT / "tests" / "staged_out_check.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "staged_out_check ok" in r.stdout, r.stdout + r.stderr
