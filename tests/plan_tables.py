"""The host table programs of the device-free plan tests (tests/<stem>.cpp over ab_opt_amd/csrc/ipa_plan.h and forward_plan.h): compiled with the host compiler, run
once, their lines handed to the test module's `table` fixture."""
import os
import shutil
import subprocess
import tempfile

TESTS = os.path.dirname(os.path.abspath(__file__))


def table_lines(stem):
    """the lines tests/<stem>.cpp prints"""
    cxx = next((c for c in ('/opt/rocm/lib/llvm/bin/clang++', shutil.which('g++'), shutil.which('clang++')) if c and os.path.exists(c)), None)
    assert cxx, 'no host C++ compiler (clang++ of the ROCm LLVM directory, g++)'
    with tempfile.TemporaryDirectory(prefix=stem) as tmp:
        exe = os.path.join(tmp, stem)
        subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', os.path.join(TESTS, stem + '.cpp'), '-o', exe], check=True)
        return subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()


def build_table(stem, Row):
    """one Row per line of a program whose lines are '|'-separated groups of integers, a name (a kernel form) among them kept as text"""
    return [Row(*(int(f) if f.lstrip('-').isdigit() else f for f in line.replace('|', ' ').split())) for line in table_lines(stem)]
