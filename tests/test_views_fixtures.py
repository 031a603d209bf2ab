"""The view fixtures of tests/golden/views/ (tools/make_view_kats.sh: the reference's own frames of one scene from 5
cameras, moved with Camera.setTransform / changeFOV) and the blob patch helper, without a GPU:
  1. the pinned oracle renders with_camera(blob, cam_v) for every fixture view and reproduces the reference's RGBA8
     bytes and f32 colours bit for bit -- which pins the fixtures, the camera numbers in cameras.json and with_camera;
  2. with_camera round-trips a blob's own camera to the identical blob, and rejects a blob without a CAMR record;
  3. every pair of views of a scene differs in at least one pixel (a camera that is ignored must fail the tests)."""
import hashlib
import struct

import numpy as np
import pytest

import views_kats as vk
from oracle import pyoracle


def _nan_equal_bits(a, b):
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def test_fixture_scenes_are_the_committed_ones():
    assert vk.scenes_on_disk() == sorted(vk.SCENES)
    for name in vk.SCENES:
        k = vk.load(name)
        assert hashlib.sha256(pyoracle.golden_scene(name)).hexdigest() == k["blob_sha256"]
        assert (k["width"], k["height"], len(k["views"])) == (20, 12, 5)
        assert (k["kind"], k["spp"]) == vk.SCENES[name]
        assert k["depth"] == pyoracle.scene_header(pyoracle.golden_scene(name))["max_depth"]


@pytest.mark.parametrize("view", range(5))
@pytest.mark.parametrize("name", sorted(vk.SCENES))
def test_oracle_renders_the_patched_blob_as_the_reference(oracle, name, view):
    k = vk.load(name)
    blob = vk.solo_blob(name, view)
    colors, rgba, _ = oracle.render(blob, k["width"], k["height"], k["spp"], k["depth"], k["kind"], k["seed"])
    grgba, gcol = vk.image(name, view)
    assert np.array_equal(rgba, grgba), f"{name} view {view}: {int((rgba != grgba).any(-1).sum())} RGBA8 pixels differ"
    assert _nan_equal_bits(colors, gcol).all(), f"{name} view {view}: f32 colours not bit-exact"


@pytest.mark.parametrize("name", sorted(vk.SCENES))
def test_view_zero_is_the_scenes_own_camera(name):
    import jsraytracer_amd as jr
    blob = pyoracle.golden_scene(name)
    cams = vk.cameras(name)
    assert cams[0] == jr.blob_camera(blob)
    assert jr.with_camera(blob, cams[0]) == blob  # the round trip
    assert all(cams[v] != cams[0] for v in range(1, 5))
    for v in range(1, 5):  # only the camera record changes, and it reads back as written
        patched = jr.with_camera(blob, cams[v])
        assert len(patched) == len(blob) and jr.blob_camera(patched) == cams[v]
        assert sum(a != b for a, b in zip(patched, blob)) <= 168
    # views 2 and 4 went through changeFOV; the depth-of-field scene's views 1 and 3 changed focus / sensor
    assert cams[2].tan_fov != cams[0].tan_fov and cams[4].tan_fov != cams[0].tan_fov and cams[1].tan_fov == cams[0].tan_fov
    if name == "BoxBall_DOF":
        assert all(c.kind == jr.renderer.CAMERA_DOF for c in cams)
        assert cams[1].focus_distance != cams[0].focus_distance and cams[3].sensor_size != cams[0].sensor_size
    else:
        assert all(c.kind == jr.renderer.CAMERA_PERSPECTIVE for c in cams)


def test_with_camera_rejects_a_blob_without_camr():
    import jsraytracer_amd as jr
    blob = bytearray(pyoracle.golden_scene("BoxBall_path"))
    cam = jr.blob_camera(bytes(blob))
    nsec = struct.unpack_from("<I", blob, 8)[0]
    for i in range(nsec):  # retag the camera section: the blob then has none
        if struct.unpack_from("<I", blob, 16 + 24 * i)[0] == 0x524D4143:
            struct.pack_into("<I", blob, 16 + 24 * i, 0x58585858)
    with pytest.raises(jr.JsrtError, match="no camera record"):
        jr.with_camera(bytes(blob), cam)
    with pytest.raises(jr.JsrtError, match="no camera record"):
        jr.blob_camera(bytes(blob))
    # ... and a CAMR section of another size
    blob = bytearray(pyoracle.golden_scene("BoxBall_path"))
    for i in range(nsec):
        if struct.unpack_from("<I", blob, 16 + 24 * i)[0] == 0x524D4143:
            struct.pack_into("<Q", blob, 16 + 24 * i + 16, 160)
    with pytest.raises(jr.JsrtError, match="168-byte camera record"):
        jr.with_camera(bytes(blob), cam)
    with pytest.raises(jr.JsrtError, match="not a JSRT"):
        jr.with_camera(b"\0" * 64, cam)


@pytest.mark.parametrize("name", sorted(vk.SCENES))
def test_every_pair_of_views_differs(name):
    imgs = [vk.image(name, v)[0] for v in range(5)]
    for a in range(5):
        for b in range(a + 1, 5):
            assert (imgs[a] != imgs[b]).any(), f"{name}: views {a} and {b} are the same image"


def test_camera_from_fov_is_the_c_tangent():
    import math

    import jsraytracer_amd as jr
    c = jr.Camera.from_fov(0.9, 1.5, np.eye(4))
    assert c.tan_fov == math.tan(0.45) and c.aspect == 1.5 and c.kind == 0
    assert c.replace(tan_fov=2.0).tan_fov == 2.0 and c.replace(tan_fov=2.0) != c
