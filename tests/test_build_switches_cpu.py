"""DESIGN.md's "Build switches" table names exactly the preprocessor symbols that conditionals in csrc/ test."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fastegnn_amd", "csrc")
SOURCES = sorted(glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.hip")))


def conditional_symbols():
    found = set()
    for path in SOURCES:
        for line in open(path):
            m = re.match(r"\s*#\s*(?:if|ifdef|ifndef|elif)\b(.*)", line)
            if m:
                found.update(re.findall(r"[A-Za-z_]\w*", m.group(1).split("//")[0]))
    # not switches: the operator, compiler-defined names, include guards
    return {s for s in found if s != "defined" and not s.startswith("__") and not s.endswith(("_H", "_H_"))}


def test_design_lists_every_build_switch_and_only_those():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = re.search(r"^## [^\n]*Build switches\n(.*?)(?=^## |\Z)", design, re.S | re.M).group(1)
    listed = set(re.findall(r"^\| `(\w+)`", section, re.M))
    assert listed, "the Build switches table has no rows"
    tested = conditional_symbols()
    assert tested - listed == set(), f"tested in csrc/ but missing from DESIGN.md 'Build switches': {sorted(tested - listed)}"
    text = "".join(open(p).read() for p in SOURCES)
    gone = {s for s in listed if not re.search(r"\b%s\b" % s, text)}
    assert gone == set(), f"listed in DESIGN.md 'Build switches' but no longer in csrc/: {sorted(gone)}"
    assert listed - tested == set(), f"listed but tested by no conditional: {sorted(listed - tested)}"
