"""ppo.c_amd has one build, and every run-time knob is documented ("One build, one knob table").

Two text checks over ppo.c_amd/csrc and ppo.c_amd/host:
  * no compile-time variants: a preprocessor conditional may test an include guard (the name the next line
    defines), __HIPCC__ or __cplusplus, and nothing else;
  * the names the code passes to getenv() are exactly the names that lead a row of the INTEGRATION.md §4 table.
"""
import pathlib
import re

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
PKG = ROOT / "ppo.c_amd"

COND = re.compile(r"^\s*#\s*(if|ifdef|ifndef|elif)\b(.*)$")
ALLOWED = {"__HIPCC__", "__cplusplus"}


@pytest.fixture(scope="module")
def sources():
    files = sorted(p for d in ("csrc", "host") for p in (PKG / d).iterdir() if p.is_file())
    assert len(files) > 20, files
    return [(p.relative_to(PKG).as_posix(), p.read_text(encoding="utf-8").splitlines()) for p in files]


def test_no_compile_time_variants(sources):
    bad = []
    for path, lines in sources:
        for n, text in enumerate(lines):
            m = COND.match(text)
            if not m:
                continue
            names = set(re.findall(r"[A-Za-z_]\w*", m.group(2))) - {"defined"}
            nxt = lines[n + 1] if n + 1 < len(lines) else ""
            guard = re.match(r"^\s*#\s*define\s+(\w+)\s*$", nxt)
            if m.group(1) == "ifndef" and guard and names == {guard.group(1)}:
                continue
            if names and names <= ALLOWED:
                continue
            bad.append(f"{path}:{n + 1}: {text.strip()}")
    assert not bad, "compile-time variants:\n" + "\n".join(bad)


def test_knobs_are_the_documented_ones(sources):
    read = {name for _, lines in sources for text in lines for name in re.findall(r'getenv\("(\w+)"\)', text)}
    assert len(read) > 10, read
    documented = set()
    in_table = False
    for text in (ROOT / "INTEGRATION.md").read_text(encoding="utf-8").splitlines():
        if text.startswith("## "):
            in_table = text.startswith("## 4.")
        if not (in_table and text.startswith("| `")):
            continue
        first = text.split("|")[1]
        documented |= {m for m in re.findall(r"`([A-Z][A-Z0-9_]*)\b[^`]*`", first)}
    assert read == documented, (f"read but not documented: {sorted(read - documented)}; "
                                f"documented but not read: {sorted(documented - read)}")
