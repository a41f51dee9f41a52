"""The per-frame colour entry points without a GPU (tests/test_colour_stream.py runs them): exported, null arguments refused before any
device call, and kinfu_stream --colour's argument and input errors (the driver reads every frame before it opens the device)."""
import ctypes as C
import os
import subprocess

import pytest

from tsdf_amd import _capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "kinfu_stream")


def test_the_library_exports_the_coloured_step_and_tracker_integrate():
    for name in ("tsdf_pipeline_step_colour", "tsdf_tracker_integrate_colour"):
        assert hasattr(_capi.lib, name) and name in _capi.EXPORTS


def test_null_arguments_are_refused():
    lib = _capi.lib
    m = _capi.CameraMatrices()
    assert lib.tsdf_pipeline_step_colour(None, C.c_void_p(16), C.c_void_p(16), C.byref(m), C.c_void_p(16), None, None, None, None) == _capi.TSDF_ERR_INVALID
    assert "null argument" in _capi.last_error()
    assert lib.tsdf_tracker_integrate_colour(None, C.byref(m), C.c_void_p(16)) == _capi.TSDF_ERR_INVALID
    assert "null argument" in _capi.last_error()


def test_kinfu_stream_colour_with_ranks_is_an_argument_error(tmp_path):
    r = subprocess.run([BIN, "-d", str(tmp_path), "--colour", "--ranks", "2"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--colour" in r.stderr, r.stderr


def test_kinfu_stream_colour_without_rgb_frames_fails_with_a_message(tmp_path):
    synth.write_tum_directory(str(tmp_path), 2, seed=0x5EED0002, width=64, height=48)
    r = subprocess.run([BIN, "-d", str(tmp_path), "--colour"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "colour image" in r.stderr and "Couldn't find file" in r.stderr, r.stderr
