"""The LAMP_* run-time switches live in ONE table (lamp_amd/csrc/core/switches.h); these are text checks of that, no GPU and no library.

The point of the second test: the bitwise A/B tests run one child process per arm of a switch.  A switch name misspelled in such a test, or
renamed in the C++, makes both arms run the default - the test passes and tests nothing."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lamp_amd", "csrc")
TABLE = os.path.join(CSRC, "core", "switches.h")

# X(member, "NAME", KIND, default, lower clamp, "what it selects")
ROW = re.compile(r'^\s*X\((\w+),\s*"(LAMP_[A-Z0-9_]+)",\s*(BOOL|INT|LETTER),\s*(.+?),\s*([\w-]+),\s*"([^"]*)"\)', re.M)

# environment names that Python reads (bench.py, lamp_amd/*.py, tests/), never the library
HARNESS = {
    "LAMP_LIB_PATH", "LAMP_RDZV_FILE", "LAMP_CONTROL_PORT", "LAMP_TESTS_NO_BUILD", "LAMP_KATS_NO_ASSERT", "LAMP_SOAK", "LAMP_SOAK_SEED",
    "LAMP_BENCH_ALSO", "LAMP_BENCH_FORCE_COMM", "LAMP_BENCH_GRAPH_UNDER_PROFILER", "LAMP_BENCH_TOP", "LAMP_EPOCH_TRACE", "LAMP_EPOCH_VARIANTS",
}


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _rows():
    return ROW.findall(_read(TABLE))


def _sources(*patterns):
    me = os.path.abspath(__file__)
    return [p for pat in patterns for p in sorted(glob.glob(os.path.join(ROOT, pat))) if os.path.abspath(p) != me]


def test_getenv_only_in_the_switch_table():
    hits = []
    for dirpath, _, names in os.walk(CSRC):
        for n in names:
            if n.endswith((".hip", ".cpp", ".h", ".hpp", ".c")) and "getenv" in _read(os.path.join(dirpath, n)):
                hits.append(os.path.relpath(os.path.join(dirpath, n), CSRC))
    assert hits == [os.path.join("core", "switches.cpp")], f"getenv outside the switch table's reader: {hits}"


def test_rows_are_described_and_unique():
    rows = _rows()
    # every X( line of the table parses: a row the pattern misses would be invisible to the checks below
    assert len(rows) == len(re.findall(r"^\s*X\(", _read(TABLE), re.M)) > 0
    names = [r[1] for r in rows]
    members = [r[0] for r in rows]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    assert len(set(members)) == len(members), sorted(m for m in members if members.count(m) > 1)
    for member, name, kind, default, clamp, doc in rows:
        assert doc.strip(), f"{name}: no description"
        assert member == name[len("LAMP_"):].lower(), f"{name}: member {member}"
    assert not HARNESS & set(names)


def test_names_set_by_tests_and_scripts_exist():
    known = {r[1] for r in _rows()} | HARNESS
    used = {}
    # tests: keyword arguments of env=dict(os.environ, LAMP_X=...), monkeypatch.setenv / delenv("LAMP_X"), os.environ["LAMP_X"] = ...
    for path in _sources("tests/*.py"):
        text = _read(path)
        found = re.findall(r"\b(LAMP_[A-Z0-9_]+)\s*=(?!=)", text)
        found += re.findall(r"""(?:setenv|delenv)\(\s*["'](LAMP_[A-Z0-9_]+)["']""", text)
        found += re.findall(r"""environ\[["'](LAMP_[A-Z0-9_]+)["']\]\s*=(?!=)""", text)
        for n in found:
            used.setdefault(n, set()).add(os.path.relpath(path, ROOT))
    # scripts: NAME=value in front of a command or in an export
    for path in _sources("scripts/*.sh", "scripts/*.py"):
        for n in re.findall(r"\b(LAMP_[A-Z0-9_]+)=", _read(path)):
            used.setdefault(n, set()).add(os.path.relpath(path, ROOT))
    assert used, "the patterns above found nothing: they no longer match how the tests set switches"
    unknown = {n: sorted(w) for n, w in used.items() if n not in known}
    assert not unknown, f"set by a test or script, read by nobody: {unknown}"
    # ... and the harness list holds only names that Python does read
    python_text = "".join(_read(p) for p in _sources("bench.py", "lamp_amd/*.py", "tests/*.py", "scripts/*.py"))
    stale = sorted(n for n in HARNESS if not re.search(r"""(?:environ|getenv)[^\n]*["']%s["']""" % n, python_text))
    assert not stale, f"harness-side names that no Python file reads: {stale}"
