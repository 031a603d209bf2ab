"""include/jsrt_views.h without a GPU: the three entry points are exported, jsrt_camera has the CAMR record's layout,
the checks that need no scene come back as -1 with their message before any HIP call, and the ABI version is unchanged."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from jsraytracer_amd import build as jb
    jb.build()
    from jsraytracer_amd import _native
    return _native.views_api()


def test_views_symbols_exported(L):
    from jsraytracer_amd import _native
    txt = open(os.path.join(ROOT, "include", "jsrt_views.h")).read()
    declared = sorted(set(re.findall(r"^int (jsrt_[a-z_]+)\s*\(", txt, re.M)))
    assert declared == sorted(_native.VIEWS_EXPORTS) == ["jsrt_render_views", "jsrt_render_views_device", "jsrt_scene_camera"]
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    for sym in declared:
        assert re.search(rf"\bT {sym}$", out, re.M), f"{sym} not exported"
    assert L.jsrt_abi_version() == 4 and _native.ABI_VERSION == 4


def test_camera_layout_is_the_camr_record():
    from jsraytracer_amd import _native
    C = _native.CameraRec
    assert ctypes.sizeof(C) == 168  # include/jsrt_scene.h jsrt_rec_camera
    assert [C.kind.offset, C.transform.offset, C.tan_fov.offset, C.aspect.offset, C.focus_distance.offset,
            C.sensor_size.offset] == [0, 8, 136, 144, 152, 160]


def test_views_refuse_a_null_scene(L):
    from jsraytracer_amd import _native
    p = _native.Params(8, 8, 1, 0, 0, 1, 0, 1)
    cam = _native.CameraRec()
    buf = (ctypes.c_uint8 * 256)()
    assert L.jsrt_render_views(None, ctypes.byref(p), ctypes.byref(cam), 1, None, buf, None, None) == -1
    assert _native.last_error() == "scene is NULL"
    assert L.jsrt_render_views_device(None, ctypes.byref(p), ctypes.byref(cam), 1, None, buf, None, None, None) == -1
    assert _native.last_error() == "scene is NULL"
    assert L.jsrt_scene_camera(None, ctypes.byref(cam)) == -1 and _native.last_error() == "scene is NULL"
