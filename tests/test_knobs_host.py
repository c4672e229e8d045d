"""The pure parsers of the runtime switches (go-kzg_amd/csrc/knobs.hpp) against the table in tests/host/knobs_test.cpp -- CPU only.

The GPU suite forces launch shapes through these switches in child processes; a switch that parses differently from what a test believes forces nothing
and the test passes for the wrong reason.  The program is a plain executable with its own main (never loaded into Python), built a second time with
AddressSanitizer and UndefinedBehaviorSanitizer: the parsers index and scan caller-supplied strings."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,flags", [("knobs_test", ["-O2"]), ("knobs_test_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])])
def test_every_parser_matches_the_table(name, flags):
    bdir = os.path.join(ROOT, "tests", "host", "_build")
    os.makedirs(bdir, exist_ok=True)
    exe = os.path.join(bdir, name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, os.path.join(ROOT, "tests", "host", "knobs_test.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and " 0 misses" in res.stdout and not res.stderr, res.stdout + res.stderr
