"""Index arithmetic of the paired-point table (go-kzg_amd/csrc/fb_pair_index.hpp: the tuple <-> entry bijection, the digit words, the recoding of two GLV
halves with independent signs) compiled for the host and checked against plain 128-bit integers by a stand-alone program,
tests/host/fb_pair_index_test.cpp: once as it is, once under AddressSanitizer + UndefinedBehaviorSanitizer.  CPU only."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host", "fb_pair_index_test.cpp")
INC = os.path.join(ROOT, "go-kzg_amd", "csrc")
OUT_DIR = os.path.join(HERE, "host", "_build")


def _build_and_run(name, flags):
    os.makedirs(OUT_DIR, exist_ok=True)
    exe = os.path.join(OUT_DIR, name)
    deps = [SRC, os.path.join(INC, "fb_pair_index.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-I", INC] + flags + ["-o", exe, SRC])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "fb_pair_index_test: ok" in r.stdout, r.stdout[-4000:]


def test_bijection_words_and_recoding_against_big_integers():
    _build_and_run("fb_pair_index_test", ["-O2"])


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers():
    _build_and_run("fb_pair_index_test_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
