"""The knob table code (shmr_amd/csrc/knobs.hpp) on the CPU: tools/knobs_check.cpp
is compiled with g++ under ASan + UBSan, once per flavour of the library, and
checks knob_set / knob_get / knob_override / knob_describe_tail on a table with
one knob of each kind against a model written out in the program (null, empty,
over-long and prefixed keys; values below, inside and above every range)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flavour", ["product", "tools"])
def test_knob_table_code_under_sanitizers(flavour, tmp_path):
    exe = str(tmp_path / "knobs_check")
    # (any sanitizer report aborts the checker and fails the test)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", *(["-DSHMR_EC_TOOLS"] if flavour == "tools" else []),
                    "-I", os.path.join(ROOT, "shmr_amd", "csrc"), os.path.join(ROOT, "tools", "knobs_check.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    assert int(r.stdout.split()[1]) > 10000
