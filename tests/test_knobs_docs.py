"""The registry of runtime switches (go-kzg_amd/csrc/knobs.hpp), README's "Environment knobs" table and the names that tests and tools set agree -- CPU only.

A switch that the code reads and the table does not list is invisible; one that a test sets and the code does not read forces nothing, and the test
passes for the wrong reason."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "go-kzg_amd", "csrc")
BINDING = {"KZG_HIP_LIB", "KZG_HIP_NO_TORCH_PRELOAD", "KZG_HIP_LIB_ALLOW_MISSING"}   # read by go-kzg_amd/__init__.py, not by the library
NOT_OURS = {"GPU_MAX_HW_QUEUES"}                                                     # the runtime's: the library does not read it
TOKEN = re.compile(r"\bKZG_(?:HIP|COALESCE)_[A-Z0-9_]*[A-Z0-9]\b")


def _read(path):
    with open(path, encoding="utf-8", errors="ignore") as f:
        return f.read()


def _registry():
    return set(re.findall(r'"(KZG_[A-Z0-9_]+)"', _read(os.path.join(CSRC, "knobs.hpp"))))


def _readme_rows():
    """the first cell of every row of the table under "## Environment knobs" """
    section = _read(os.path.join(ROOT, "README.md")).split("## Environment knobs", 1)[1].split("\n## ", 1)[0]
    rows = [line.split("|")[1] for line in section.splitlines() if line.startswith("|")]
    return rows[2:]   # less the header and the rule


def test_the_registry_defines_switches():
    names = _registry()
    assert len(names) >= 40 and "KZG_HIP_FR_FFT" in names and "KZG_COALESCE_SIM_MAX_BUFS" in names, sorted(names)
    assert not names & (BINDING | NOT_OURS), sorted(names & (BINDING | NOT_OURS))


def test_readme_lists_every_switch_once():
    cells = [re.findall(r"`([A-Z][A-Z0-9_]+)`", cell) for cell in _readme_rows()]
    assert all(len(c) == 1 for c in cells), [c for c in cells if len(c) != 1]   # one row per switch, its full name in the first cell
    listed = [c[0] for c in cells]
    assert sorted(set(listed)) == sorted(listed), sorted(n for n in set(listed) if listed.count(n) > 1)
    assert set(listed) - BINDING - NOT_OURS == _registry(), (sorted(set(listed) - BINDING - NOT_OURS - _registry()), sorted(_registry() - set(listed)))


def test_only_the_registry_reads_the_environment():
    readers = [f for f in sorted(os.listdir(CSRC)) if os.path.isfile(os.path.join(CSRC, f)) and "getenv(" in _read(os.path.join(CSRC, f))]
    assert readers == ["knobs.hpp"], readers


def test_tests_and_tools_name_only_switches_that_exist():
    # what else carries these prefixes: the constants of the public header and the compile-time macros of the sources
    known = _registry() | BINDING | set(re.findall(r"#\s*define\s+(KZG_HIP_\w+)", _read(os.path.join(ROOT, "include", "kzg_hip.h"))))
    for f in os.listdir(CSRC):
        if os.path.isfile(os.path.join(CSRC, f)):
            known |= set(re.findall(r"#\s*(?:define|ifdef|ifndef)\s+(KZG_\w+)", _read(os.path.join(CSRC, f))))
    files = [os.path.join(ROOT, "bench.py")]
    for top in ("tests", "tools", "benchlib"):
        for d, dirs, names in os.walk(os.path.join(ROOT, top)):
            dirs[:] = [x for x in dirs if x not in ("_build", "__pycache__", "_variants")]
            files += [os.path.join(d, n) for n in names]
    unknown = {}
    for path in files:
        for tok in set(TOKEN.findall(_read(path))) - known:
            unknown.setdefault(tok, []).append(os.path.relpath(path, ROOT))
    assert not unknown, unknown
