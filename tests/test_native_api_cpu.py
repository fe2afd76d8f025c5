"""The native entry points (``rdp_*``) are declared once: in csrc/rdp_api.h and csrc/rdp_host_api.h (C linkage) and,
for the conv plan that rdp_api.h includes, in csrc/conv_plan.h.

With C linkage neither compiler nor linker compares a hand-copied prototype with its definition, so a copy that
drifts still links and shifts every argument after the change. The headers make the compiler compare -- as long as
no copy exists beside them and every definer includes them. This is a source-text check of exactly that.
"""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ("rdp_api.h", "rdp_host_api.h", "conv_plan.h")
# `<type> rdp_name(` with nothing but type tokens before the name on its line: a declaration or a definition
HEAD = re.compile(r'^[ \t]*(?:extern "C" )?((?:[\w:]+[ \t\*&]+)+)(rdp_\w+)[ \t]*\(', re.M)


def _entries(text):
    """(name, '{' for a definition / ';' for a bodiless declaration) of every rdp_* function head in text"""
    for m in HEAD.finditer(text):
        if m.group(1).split()[0] in ("return", "else", "case", "new", "delete", "throw"):
            continue
        i, depth = m.end() - 1, 0
        while True:
            depth += {"(": 1, ")": -1}.get(text[i], 0)
            i += 1
            if depth == 0:
                break
        tail = text[i:].lstrip()
        if tail[:1] in ("{", ";"):
            yield m.group(2), tail[0]


def _sources():
    pats = ("csrc/*.hip", "csrc/*.cpp", "csrc/*.h", "tests/native/*")
    return sorted(p for pat in pats for p in glob.glob(os.path.join(ROOT, pat)) if os.path.basename(p) not in HEADERS)


def test_headers_declare_the_entry_points():
    for h in HEADERS:  # the check below means something only if the headers are what declares them
        assert sum(kind == ";" for _, kind in _entries(open(os.path.join(ROOT, "csrc", h)).read())) >= 10, h


def test_no_prototype_outside_the_two_headers():
    copies = [(os.path.relpath(p, ROOT), name) for p in _sources() for name, kind in _entries(open(p).read())
              if kind == ";"]
    assert not copies, f"hand-written rdp_* prototypes (declare them in csrc/rdp_api.h / rdp_host_api.h / conv_plan.h): {copies}"


def test_every_definer_includes_a_header():
    missing = []
    for p in _sources():
        text = open(p).read()
        if os.path.dirname(p).endswith("csrc") and any(kind == "{" for _, kind in _entries(text)):
            if not any(f'#include "{h}"' in text for h in HEADERS):
                missing.append(os.path.relpath(p, ROOT))
    assert not missing, f"files that define rdp_* entry points without including their declaration: {missing}"
