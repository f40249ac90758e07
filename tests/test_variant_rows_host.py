"""The rules of variant ranges and variant lists on the host alone: tests/host/variant_rows_main.cpp includes only
plinking_duck_amd/csrc/variant_rows.hpp (no HIP, no handle types) and is built with AddressSanitizer + UBSan on the
CPU.  What it asserts is listed in its source; tests/test_variant_shapes.py pins the same rules through every entry
point on the GPU."""

import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "plinking_duck_amd", "csrc")


def test_variant_rows_resolver_under_sanitizers(tmp_path):
    exe = str(tmp_path / "variant_rows_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", SRC, os.path.join(ROOT, "tests", "host", "variant_rows_main.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "variant rows ok" in r.stdout
