"""The lazy F_p cores and the mixed addition built on them (field.hpp / g1.hpp: g1x_madd_fast on entries as stored and negated, P = +-Q) compiled
for the host and checked against plain big integers by a stand-alone program, tests/host/fp_lazy_trims_test.cpp: once as it is, once under
AddressSanitizer + UndefinedBehaviorSanitizer.  CPU only."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host", "fp_lazy_trims_test.cpp")
INC = os.path.join(ROOT, "go-kzg_amd", "csrc")
OUT_DIR = os.path.join(HERE, "host", "_build")


def _build_and_run(name, flags):
    os.makedirs(OUT_DIR, exist_ok=True)
    exe = os.path.join(OUT_DIR, name)
    deps = [SRC, os.path.join(INC, "field.hpp"), os.path.join(INC, "g1.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-I", INC] + flags + ["-o", exe, SRC])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "fp_lazy_trims_test: ok" in r.stdout, r.stdout[-4000:]


def test_lazy_cores_and_mixed_addition_against_big_integers():
    _build_and_run("fp_lazy_trims_test", ["-O2"])


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers():
    _build_and_run("fp_lazy_trims_test_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
