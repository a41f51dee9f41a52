"""The weight cap's surface without a GPU: the two entry points are declared, exported and bound, kinfu_stream lists its option, and the
header states the rule (include/tsdf_amd.h, "weight cap")."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tsdf_amd.h")
LIB = os.path.join(ROOT, "tsdf_amd", "lib", "libtsdf_hip.so")
BIN = os.path.join(ROOT, "build", "kinfu_stream")
SYMBOLS = ("tsdf_volume_set_weight_cap", "tsdf_volume_weight_cap")


def header_text():
    with open(HEADER) as f:
        return f.read()


def test_the_entry_points_are_declared_and_exported():
    text = header_text()
    assert re.search(r"int\s+tsdf_volume_set_weight_cap\s*\(\s*tsdf_volume\s*\*\s*volume\s*,\s*uint32_t\s+cap\s*\)\s*;", text)
    assert re.search(r"int\s+tsdf_volume_weight_cap\s*\(\s*const\s+tsdf_volume\s*\*\s*volume\s*,\s*uint32_t\s*\*\s*cap\s*\)\s*;", text)
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for s in SYMBOLS:
        assert s in exported, s + " is not exported by libtsdf_hip.so"


def test_the_entry_points_are_bound_in_python():
    from tsdf_amd import _capi, api
    for s in SYMBOLS:
        assert getattr(_capi.lib, s).argtypes is not None, s
    assert callable(api.TSDFVolume.set_weight_cap) and callable(api.TSDFVolume.weight_cap)


def test_kinfu_stream_lists_the_option():
    assert os.path.exists(BIN), "build/kinfu_stream missing: run `make cpptest` (build() does)"
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert "--weight-cap" in r.stdout + r.stderr
    r = subprocess.run([BIN, "-d", "nowhere", "--weight-cap", "65536"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "65535" in r.stderr


def test_the_header_states_the_stored_weight_rule():
    text = header_text()
    group = text[text.index("---- weight cap"):text.index("---- colour fusion")]
    flat = " ".join(group.split())
    assert "stored_weight = (prior_weight + 1.0f > (float)c) ? (float)c : prior_weight + 1.0f" in flat
    assert "new_distance = (prior_distance * prior_weight + tsdf * 1.0f) / (prior_weight + 1.0f)" in flat
    assert "divisor is always prior_weight + 1" in flat
    assert "TSDF_ERR_INVALID" in flat and "65535" in flat
