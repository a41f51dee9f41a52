"""The parser of include/tsdf_amd.h that the symbol tests of columns, esdf, explore, frame_diff, objects, reach and snapshot share
(tests/test_capi_*_symbols.py).  Each test keeps its own EXPECTED table and its own assertions."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declarations(expected):
    """The header's text without comments, and name -> (return type, argument types with the parameter names taken out) of every
    declaration named in `expected`."""
    text = open(os.path.join(ROOT, "include", "tsdf_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"\b(int|void)\s+(tsdf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        if name not in expected:
            continue
        types = []
        for a in args.split(","):
            a = " ".join(a.split())
            m = re.match(r"^(.*?)([A-Za-z_][A-Za-z0-9_]*)(\[\d+\])?$", a)
            types.append((m.group(1).strip() + (" " + m.group(3) if m.group(3) else "")).strip())
        out[name] = (ret, types)
    return text, out
