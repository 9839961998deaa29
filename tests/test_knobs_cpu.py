"""The MIFT_* environment switches the package reads are exactly the ones docs/KNOBS.md lists."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import mift  # noqa: E402  (tests/conftest.py puts the repository root on sys.path)

PKG = os.path.join(ROOT, mift.PKG_DIRNAME)
# a name in env-read position: getenv("MIFT_X"), the native helper mift_env_int("MIFT_X", ...),
# os.environ.get("MIFT_X"...), os.environ["MIFT_X"], os.environ.setdefault("MIFT_X", ...)
READ = re.compile(r'(?:getenv\(|mift_env_int\(|os\.environ\.get\(|os\.environ\[|os\.environ\.setdefault\()\s*'
                  r'"(MIFT_[A-Z0-9_]+)"')
MAX_KNOBS = 40


def _sources(top, exts):
    for dp, _, fs in os.walk(top):
        for f in sorted(fs):
            if f.endswith(exts):
                yield os.path.join(dp, f)


def _read(path):
    with open(path, encoding="utf-8") as fh:
        return fh.read()


def _names_read():
    names = set()
    for path in _sources(PKG, (".py", ".cpp", ".h", ".hip")):
        names.update(READ.findall(_read(path)))
    return names


def _names_documented():
    rows = re.findall(r"^\|\s*`(MIFT_[A-Z0-9_]+)`\s*\|", _read(os.path.join(ROOT, "docs", "KNOBS.md")), re.M)
    assert len(rows) == len(set(rows)), "docs/KNOBS.md lists a switch twice"
    return set(rows)


def test_switches_read_are_the_documented_ones():
    read, doc = _names_read(), _names_documented()
    assert read - doc == set(), f"read by the package but missing from docs/KNOBS.md: {sorted(read - doc)}"
    assert doc - read == set(), f"listed in docs/KNOBS.md but read nowhere: {sorted(doc - read)}"
    assert len(read) <= MAX_KNOBS, f"{len(read)} switches (limit {MAX_KNOBS}): {sorted(read)}"


def test_knobs_table_rows_are_complete():
    classes = ("user/config", "test-forced path", "A/B between two shipped paths")
    for line in _read(os.path.join(ROOT, "docs", "KNOBS.md")).splitlines():
        if re.match(r"^\|\s*`MIFT_", line):
            cells = [c.strip() for c in line.strip().strip("|").split("|")]
            assert len(cells) == 5 and all(cells), line
            assert cells[4] in classes, line


def test_no_native_switch_read_is_cached_in_a_static():
    pat = re.compile(r"static[^;]*(?:getenv|mift_env_int)")
    hits = [os.path.relpath(p, ROOT) for p in _sources(os.path.join(PKG, "csrc"), (".cpp", ".h", ".hip"))
            if pat.search(_read(p))]
    assert hits == [], f"static-cached getenv in {hits}"
