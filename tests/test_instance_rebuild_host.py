"""Rebuilding the top tree of an instanced scene (include/pathed_hip.h: pathed_hip_scene_rebuild_top),
the part that needs no GPU: the entry point is declared, bound and exported, and the ABI version stays."""
import ctypes as C
import os
import re

from pathed_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include", "pathed_hip.h")).read()


def test_the_header_declares_it_and_the_abi_version_stays():
    assert re.search(r"int pathed_hip_scene_rebuild_top\(PathedScene \*scene, int32_t builder, float \*device_ms\);", header())
    assert re.search(r"#define PATHED_ABI_VERSION 4\b", header())   # one new function, no struct changes


def test_the_binding_lists_it():
    assert "pathed_hip_scene_rebuild_top" in _capi.HIP_SYMBOLS


def test_the_library_exports_it():
    lib = C.CDLL(_capi.hip_library_path())
    assert hasattr(lib, "pathed_hip_scene_rebuild_top")

