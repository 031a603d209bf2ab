"""TEST INFRASTRUCTURE: readers of tests/golden/views/ (tools/make_view_kats.sh), shared by test_views_fixtures.py and
test_gpu_views.py: per scene cameras.json (the reference's live camera numbers per view and the render's
parameters) and per view the reference's RGBA8 bytes and f32 colours."""
import json
import os

import numpy as np

from oracle import pyoracle

VIEWS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "views")
# scene -> (renderer kind, spp): one scene per code path (hybrid chain, plain chain, tree, persistent march, BVH, DOF)
SCENES = {"cornell_box_path": (1, 3), "BoxBall_path": (1, 2), "Aggregates": (0, 1), "SDF_Menger": (1, 1),
          "bunny": (2, 2), "BoxBall_DOF": (1, 2)}
_kats, _cams, _images = {}, {}, {}


def scenes_on_disk():
    return sorted(os.listdir(VIEWS))


def load(name):
    if name not in _kats:
        with open(os.path.join(VIEWS, name, "cameras.json")) as f:
            _kats[name] = json.load(f)
    return _kats[name]


def cameras(name):
    """The scene's 5 fixture cameras as jsraytracer_amd.Camera objects (view 0: the scene's own)."""
    if name not in _cams:
        import jsraytracer_amd as jr
        _cams[name] = [jr.Camera(v["transform"], v["tan_fov"], v["aspect"], v["kind"], v["focus_distance"], v["sensor_size"])
                       for v in load(name)["views"]]
    return _cams[name]


def image(name, view):
    """(rgba u8 [H, W, 4], colors f32 [H, W, 4]) of a fixture view, read-only."""
    if (name, view) not in _images:
        k = load(name)
        shape = (k["height"], k["width"], 4)
        rgba = np.fromfile(os.path.join(VIEWS, name, f"view{view}.rgba"), np.uint8).reshape(shape)
        col = np.fromfile(os.path.join(VIEWS, name, f"view{view}.f32"), np.float32).reshape(shape)
        rgba.setflags(write=False)
        col.setflags(write=False)
        _images[name, view] = (rgba, col)
    return _images[name, view]


def solo_blob(name, view, cams=None):
    """The scene whose CAMR record is the view's camera: what a view is, by definition, a render of."""
    import jsraytracer_amd as jr
    return jr.with_camera(pyoracle.golden_scene(name), (cams or cameras(name))[view])
