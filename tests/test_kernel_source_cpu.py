"""The kernel source carries no compile-time experiment switches, and no tool asks for one.

Rounds 2-4 left timing-only and rejected variants inside the hottest device functions as `#ifdef` blocks; they were taken
out once their records were in `profiles/` (profiles/README.md lists which switch produced which record).  Two checks on
the source text keep them from growing back -- neither looks at generated code:

  * every macro that an `#if` / `#ifdef` / `#ifndef` / `#elif` of the HIP translation unit tests is on an explicit list:
    include guards, the compiler's own macros, the shipped `exact` build and the four tuning constants whose every value
    gives valid results;
  * no file under tools/ names a CPK_* macro that cpecan_amd/csrc does not define.

A new switch that belongs in the product is added to ALLOWED here, with its reason; an experiment goes into a file of
its own under tools/ (as tools/ticket_forms.hip, tools/omod_check.hip).
"""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "cpecan_amd" / "csrc"
KERNEL_SOURCES = sorted(CSRC.glob("*.hip")) + sorted(CSRC.glob("*.inl")) + [CSRC / "cpecan_internal.h"]

ALLOWED = {
    # include guards
    "CPECAN_INTERNAL_H_",
    "CPECAN_BAND_INL_",
    # the compiler's
    "__HIPCC__",
    "__cplusplus",
    "__HIP_DEVICE_COMPILE__",
    "__gfx950__",
    "__gfx942__",
    # a shipped, tested build (make exact, tests/test_gpu_exact.py)
    "CPK_LOGADD_EXACT",
    # tuning constants: every value gives valid results
    "CPK_SWEEP_WAVES",
    "CPK_PACKED_WAVES",
    "CPK_EXP_DEPTH",
    "CPK_ABS_SLACK",
}

_CONDITIONAL = re.compile(r"^[ \t]*#[ \t]*(if|ifdef|ifndef|elif)\b(.*)$", re.M)
_IDENT = re.compile(r"[A-Za-z_]\w*")


def _logical_lines(text):
    return text.replace("\\\n", " ")


def _tested_macros(text):
    names = set()
    for m in _CONDITIONAL.finditer(_logical_lines(text)):
        expr = re.sub(r"//.*|/\*.*?\*/", "", m.group(2))
        names |= {n for n in _IDENT.findall(expr) if n != "defined"}
    return names


def test_conditionals_test_only_listed_macros():
    assert len(KERNEL_SOURCES) > 5 and all(p.is_file() for p in KERNEL_SOURCES)
    found = {}
    for p in KERNEL_SOURCES:
        for name in _tested_macros(p.read_text()):
            found.setdefault(name, []).append(p.name)
    # the scan sees what it should: the exact build's switch and the architecture guard are there
    assert "CPK_LOGADD_EXACT" in found and "__gfx950__" in found
    extra = {n: f for n, f in found.items() if n not in ALLOWED}
    assert not extra, "compile-time switches outside the allow-list: %r" % extra


def test_tools_name_only_macros_the_source_defines():
    defined = set()
    for p in CSRC.iterdir():
        if p.is_file() and p.suffix in (".hip", ".inl", ".h", ".c"):
            defined |= set(re.findall(r"^[ \t]*#[ \t]*define[ \t]+(CPK_[A-Z0-9_]+)", p.read_text(), re.M))
    assert "CPK_WAVE" in defined and "CPK_LOGADD_EXACT" in defined
    stale = {}
    tools = [p for p in sorted((ROOT / "tools").rglob("*")) if p.is_file()]
    assert tools
    for p in tools:
        unknown = set(re.findall(r"\bCPK_[A-Z0-9_]+", p.read_text(errors="replace"))) - defined
        if unknown:
            stale[str(p.relative_to(ROOT))] = sorted(unknown)
    assert not stale, "tools name CPK_ macros that cpecan_amd/csrc does not define: %r" % stale
