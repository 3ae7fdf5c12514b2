"""csrc/build.sh is the only place that names the library's translation units.

(a) every csrc/*.hip and csrc/*.cpp is compiled by build.sh, and build.sh names no file that does not exist;
(b) no script under tools/ carries a source list of its own: a diagnostic or A/B build calls build.sh (AQG_EXTRA_FLAGS, OUT, OBJDIR,
    AQG_REPLACE).  Ten tools once kept the list of five rounds before and built libraries that could no longer link, with the
    compiler's errors thrown away.
"""
import glob
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "alphaquoridorgnn_amd", "csrc")


def _build_sh():
    with open(os.path.join(CSRC, "build.sh")) as f:
        return f.read()


def test_build_sh_compiles_every_source_file_and_names_no_other():
    text = _build_sh()
    loops = re.findall(r"^for f in ([\w ]+); do$", text, flags=re.M)
    assert len(loops) == 1, "build.sh: expected exactly one `for f in <units>; do` list"
    units = loops[0].split()
    assert len(units) == len(set(units)), "a unit is listed twice"
    named = {u + ".hip" for u in units} | set(re.findall(r"-c (\w+\.cpp)\b", text))
    present = {os.path.basename(p) for ext in ("*.hip", "*.cpp") for p in glob.glob(os.path.join(CSRC, ext))}
    assert named - present == set(), f"build.sh names files that do not exist: {sorted(named - present)}"
    assert present - named == set(), f"build.sh does not compile: {sorted(present - named)}"


def test_no_tool_keeps_a_source_list_of_its_own():
    offenders = []
    for path in sorted(glob.glob(os.path.join(REPO, "tools", "*.py")) + glob.glob(os.path.join(REPO, "tools", "*.sh"))):
        with open(path, errors="replace") as f:
            lines = f.read().splitlines()
        for no, line in enumerate(lines, 1):
            if "capi.hip" in line:
                offenders.append(f"{os.path.relpath(path, REPO)}:{no}: names capi.hip")
            # the command may be split over adjacent string literals: a compiler on this line or the one before
            # (a stand-alone probe under tools/ubench/ is nobody's translation unit)
            elif re.search(r"(?<!ubench/)\b\w+\.hip\b", line) and any(re.search(r"\bhipcc\b", l) for l in lines[max(0, no - 2):no]):
                offenders.append(f"{os.path.relpath(path, REPO)}:{no}: compiles a .hip file itself")
    assert not offenders, "tools must build the library through csrc/build.sh:\n" + "\n".join(offenders)
