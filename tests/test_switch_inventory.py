"""The environment switches of the package and its library are exactly those documented in INTEGRATION.md section 4.

A `DR_*` variable counts when the sources READ it (os.environ / getenv); error codes (DR_EINVAL ...) and compile-time defines are
not switches.  Reads under `#ifdef DR_*_ABLATE` exist only in experiment builds and are left out.  A new switch has to be added to
the table -- with the test that sets it -- or this fails; so does a table row whose switch is gone."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep_recommenders_amd")
PY_READ = re.compile(r"""environ(?:\.get\(|\[)\s*["'](DR_\w+)["']|getenv\(\s*["'](DR_\w+)["']|["'](DR_\w+)["']\s+(?:not\s+)?in\s+\w*\.environ""")
C_READ = re.compile(r'getenv\(\s*"(DR_\w+)"')


def _python_reads():
    names = set()
    for path in glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True):
        for m in PY_READ.finditer(open(path).read()):
            names.add(next(g for g in m.groups() if g))
    return names


def _c_reads():
    names = set()
    for path in glob.glob(os.path.join(PKG, "csrc*", "**", "*"), recursive=True):
        if not os.path.isfile(path):
            continue
        ablate = []                  # one entry per open #if: True while inside the arm an experiment define switches on
        for line in open(path, errors="replace"):
            d = line.strip()
            if d.startswith("#if"):
                ablate.append(re.match(r"#\s*ifdef\s+DR_\w*ABLATE\b", d) is not None)
            elif d.startswith(("#else", "#elif")) and ablate:
                ablate[-1] = False
            elif d.startswith("#endif") and ablate:
                ablate.pop()
            elif not any(ablate):
                names.update(C_READ.findall(line))
    return names


def _documented():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    return set(re.findall(r"^\s*\|\s*`(DR_\w+)`\s*\|", text, re.M))


def test_the_readers_find_the_known_switches():
    assert {"DR_FUSE_K3", "DR_PREFETCH_EARLY", "DR_HIPCC_EXTRA"} <= _python_reads()
    assert {"DR_GEMM_SPLIT", "DR_K4_DETERMINISTIC", "DR_BF3_RS64"} <= _c_reads()
    assert "DR_BF3_RS_DBG" not in _c_reads() and "DR_EINVAL" not in _c_reads()      # an ablation read; an error code


def test_switches_read_equal_switches_documented():
    read, documented = _python_reads() | _c_reads(), _documented()
    assert read == documented, "read but not in INTEGRATION.md's table: %s; in the table but read nowhere: %s" % (
        sorted(read - documented), sorted(documented - read))
