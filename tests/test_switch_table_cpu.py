"""README.md's table of environment switches names exactly the SA_HIP_* variables the sources read: the library through
getenv / diag_env (suffixarray_amd/csrc, include), the Python layer through os.environ."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _files(*patterns):
    return [p for pat in patterns for p in sorted(glob.glob(os.path.join(ROOT, pat))) if os.path.isfile(p)]


def test_readme_table_lists_every_switch_the_sources_read():
    read = set()
    for p in _files("suffixarray_amd/csrc/*", "include/*"):
        read |= {m[1] for m in re.findall(r'(diag_env|getenv)\("(SA_HIP_[A-Z0-9_]+)"\)', _read(p))}
    for p in _files("suffixarray_amd/*.py", "suffixarray_amd/*.pyx"):
        read |= set(re.findall(r'os\.environ(?:\.get\(|\[)\s*["\'](SA_HIP_[A-Z0-9_]+)["\']', _read(p)))
    table = re.findall(r"^\| `(SA_HIP_[A-Z0-9_]+)` \|", _read(os.path.join(ROOT, "README.md")), re.M)
    assert len(table) == len(set(table)), sorted(n for n in set(table) if table.count(n) > 1)
    assert set(table) == read, {"read, not in the table": sorted(read - set(table)), "in the table, not read": sorted(set(table) - read)}
    assert {"SA_HIP_DIAG", "SA_HIP_LIB", "SA_HIP_ALLOW_HOST"} <= read
