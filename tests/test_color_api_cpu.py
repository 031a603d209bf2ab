"""include/jsrt_color.h without a GPU: the three entry points are exported, every argument they refuse comes back
as -1 with its message before any HIP call, n = 0 is answered without a device, and the ABI version is unchanged."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from jsraytracer_amd import build as jb
    jb.build()
    from jsraytracer_amd import _native
    return _native.color_api()


def _err():
    from jsraytracer_amd import _native
    return _native.last_error()


def test_color_symbols_exported(L):
    from jsraytracer_amd import _native
    txt = open(os.path.join(ROOT, "include", "jsrt_color.h")).read()
    declared = sorted(set(re.findall(r"^int (jsrt_[a-z_]+)\s*\(", txt, re.M)))
    assert declared == sorted(_native.COLOR_EXPORTS) == ["jsrt_camera_rays", "jsrt_color", "jsrt_color_device"]
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    for sym in declared:
        assert re.search(rf"\bT {sym}$", out, re.M), f"{sym} not exported"
    assert L.jsrt_abi_version() == 4 and _native.ABI_VERSION == 4


def test_color_params_layout():
    from jsraytracer_amd import _native
    assert ctypes.sizeof(_native.ColorParams) == 32
    assert [_native.ColorParams.max_depth.offset, _native.ColorParams.seed.offset, _native.ColorParams.sample0.offset,
            _native.ColorParams.spp.offset, _native.ColorParams.max_paths.offset] == [0, 4, 8, 12, 16]


@pytest.mark.parametrize("fn", ["jsrt_color", "jsrt_color_device"])
def test_color_refuses_bad_arguments(L, fn):
    from jsraytracer_amd import _native
    rays = np.zeros((4, 6), np.float32)
    out = np.zeros((4, 2, 3), np.float32)
    cp = _native.ColorParams(-1, 1, 0, 2, 0)
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: every check below comes before the scene is read

    def call(scene, r, n, params, o):
        args = [scene, r, None, n, params, o] + ([None] if fn == "jsrt_color_device" else []) + [None]
        return getattr(L, fn)(*args)

    assert call(None, rays.ctypes.data, 4, ctypes.byref(cp), out.ctypes.data) == -1 and _err() == "scene is NULL"
    assert call(fake, None, 4, ctypes.byref(cp), out.ctypes.data) == -1 and _err() == "rays is NULL"
    assert call(fake, rays.ctypes.data, 4, None, out.ctypes.data) == -1 and _err() == "params is NULL"
    assert call(fake, rays.ctypes.data, 4, ctypes.byref(cp), None) == -1 and _err() == "out_rgb is NULL"
    # n * spp above 2^31 (n alone, and through spp); exactly 2^31 passes this check and meets the next one
    big = _native.ColorParams(17, 1, 0, 2, 0)
    assert call(fake, rays.ctypes.data, (1 << 30) + 1, ctypes.byref(big), out.ctypes.data) == -1
    assert _err() == "n * spp above 2^31 paths is not supported"
    assert call(fake, rays.ctypes.data, (1 << 31) + 1, ctypes.byref(_native.ColorParams(17, 1, 0, 0, 0)), out.ctypes.data) == -1
    assert _err() == "n * spp above 2^31 paths is not supported"
    assert call(fake, rays.ctypes.data, 1 << 30, ctypes.byref(big), out.ctypes.data) == -1
    assert _err() == "maxRecursionDepth above 16 is not supported"
    # n = 0: nothing to do, whatever else is passed, and no device is touched
    assert call(None, None, 0, None, None) == 0
    assert call(fake, rays.ctypes.data, 0, ctypes.byref(cp), out.ctypes.data) == 0


def test_camera_rays_refuses_bad_arguments(L):
    from jsraytracer_amd import _native
    p = _native.Params(8, 8, 1, 0, 0, 1, 0, 1)
    assert L.jsrt_camera_rays(None, ctypes.byref(p), 0, None) == -1 and _err() == "scene is NULL"
