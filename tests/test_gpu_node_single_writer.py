"""A lit node's record written once, and the last level shaded without child directions.

Where a batch's shadow kernel is k_shadow_node (a flat scene, one area light of 2..4 samples on a bucketed hand-off;
run_batch's node_form), k_shade no longer writes the record of a lit node whose ambient is its material's constant:
k_shadow_node writes {ambient + light sum, info} from the hand-off tag alone (WArgs::node_single, HAND_AMB).  And
the level whose children are not cast (k_shade<LAST>) computes their count and factors without their directions.
Every frame here must equal the oracle bit for bit, RGBA8 and the f32 colours, with the node form asked for
(JSRT_SHADOW_NODE=1) and forced off (=0: the lane-per-sample k_shadow, the double write), on 20x12 at 2 spp and on
1x1 at 3 spp:

  cornell_box_path at depths 1 (every node a last-level node), 2 (one level of each kind) and 8: path-tracing walls
      with a constant ambient 0 (single writer) and the floor, whose ambient chain is a checkerboard scaled by 0 --
      not a constant, so it keeps its record from k_shade (HAND_AMB);
  amb_const: the same scene with every ambient scale 0.25 (walls: a non-zero constant; floor: a non-zero checkerboard);
  amb_checker: the same scene with only the floor's ambient scale 0.5 (the non-constant ambient alone);
  cornell_box: Phong walls with a constant ambient 0.1 under the same area light;
  heart (a Sphere area light) and refraction_path (two point lights): never the node form, the double write stays.

The redo paths: the 20x12 cornell frame with JSRT_POOL_FACTOR=1 and with JSRT_BOUND_MARGIN=0.5
(tests/test_gpu_redo_streams.py), at 6 spp in three batches of 768 path slots -- a learned bound is never below 256
rays (level_bounds), so a batch needs more than 256 live chains at level 1 for the halved bound to be outgrown: a
poisoned frame (LVL_FLAG / LVL_UNDER), whose unshaded nodes hold no record at all, is redone and not resolved."""
import gzip
import json
import os

import numpy as np
import pytest

from oracle import pyoracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JDIR = os.path.join(ROOT, "tests", "golden", "json")
FRAMES = [(20, 12, 2), (1, 1, 3)]


def _cornell_doc():
    with gzip.open(os.path.join(JDIR, "cornell_box_path.json.gz"), "rb") as f:
        return json.loads(f.read())


def _ambients(doc):
    """(object index, the material's ambient record) of every object of the world"""
    objs = doc["_v"]["renderer"]["_v"]["world"]["_v"]["objects"]["_v"]
    return [(i, o["_v"]["material"]["_v"]["ambient"]) for i, o in enumerate(objs)
            if isinstance(o["_v"].get("material"), dict) and "_v" in o["_v"]["material"]
            and "ambient" in o["_v"]["material"]["_v"]]


def _amb_const():
    doc = _cornell_doc()
    amb = _ambients(doc)
    assert len(amb) >= 2
    for _, a in amb:
        assert "_scale" in a["_v"]
        a["_v"]["_scale"] = 0.25
    return doc


def _amb_checker():
    doc = _cornell_doc()
    (floor,) = [a for i, a in _ambients(doc) if i == 0]  # object 0: the checkerboard floor
    floor["_v"]["_scale"] = 0.5
    return doc


DERIVED = {"amb_const": _amb_const, "amb_checker": _amb_checker}
# (scene, depth; None: the scene's own)
SCENES = [("cornell_box_path", 1), ("cornell_box_path", 2), ("cornell_box_path", 8), ("amb_const", 3), ("amb_checker", 3),
          ("cornell_box", None), ("heart", 3), ("refraction_path", 3)]


@pytest.fixture(scope="module")
def jr():
    import jsraytracer_amd as jr
    return jr


_blobs, _oracle = {}, {}


def _blob(jr, name):
    if name not in _blobs:
        _blobs[name] = (jr.blob_from_json(json.dumps(DERIVED[name]()), [])[0] if name in DERIVED
                        else pyoracle.golden_scene(name))
    return _blobs[name]


def _reference(blob, name, W, H, spp, depth, seed):
    key = (name, W, H, spp, depth, seed)
    if key not in _oracle:
        ocol, orgba, _ = pyoracle.render(blob, W, H, spp, depth, 1, seed)
        ocol.setflags(write=False)
        orgba.setflags(write=False)
        _oracle[key] = (ocol, orgba)
    return _oracle[key]


def _equal(rgba, colors, orgba, ocol, label):
    bad = (rgba != orgba).any(-1)
    a, b = colors[..., :3], ocol[..., :3]
    fin = np.isfinite(a) & np.isfinite(b)
    print(f"{label}: {int(bad.sum())} RGBA8 pixels differ, max |dRGB| {float(np.abs(a[fin] - b[fin]).max()) if fin.any() else 0.0:.3g}, "
          f"{int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).sum())} f32 words differ")
    assert not bad.any(), f"{label}: {int(bad.sum())} RGBA8 pixels differ"
    assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)), f"{label}: f32 colours differ"


@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f"{f[0]}x{f[1]}_s{f[2]}")
@pytest.mark.parametrize("scene", SCENES, ids=lambda s: f"{s[0]}_d{s[1]}")
def test_single_writer_and_last_level_match_oracle(jr, monkeypatch, scene, frame):
    name, depth = scene
    W, H, spp = frame
    blob = _blob(jr, name)
    if depth is None:
        depth = pyoracle.scene_header(blob)["max_depth"]
    ocol, orgba = _reference(blob, name, W, H, spp, depth, 7)
    if name != "heart" and (W, H) != (1, 1):
        assert int((orgba[..., :3] > 0).any(-1).sum()) > W * H // 8  # a lit image, not a black one
    for form in ("0", "1"):
        monkeypatch.setenv("JSRT_SHADOW_NODE", form)
        rgba, colors, st = jr.Scene(blob, device=0).render(W, H, spp, depth, 1, 7)
        _equal(rgba, colors, orgba, ocol, f"{name} d{depth} {W}x{H} JSRT_SHADOW_NODE={form}")
        assert st["samples"] == W * H * spp


@pytest.mark.parametrize("knob", [("JSRT_POOL_FACTOR", "1"), ("JSRT_BOUND_MARGIN", "0.5")], ids=lambda k: "=".join(k))
def test_poisoned_frame_is_redone_not_resolved(jr, monkeypatch, knob):
    W, H, spp = FRAMES[0][0], FRAMES[0][1], 6
    blob = _blob(jr, "cornell_box_path")
    ocol, orgba = _reference(blob, "cornell_box_path", W, H, spp, 8, 7)
    monkeypatch.setenv(*knob)
    monkeypatch.setenv("JSRT_SHADOW_NODE", "1")
    rgba, colors, st = jr.Scene(blob, device=0).render(W, H, spp, 8, 1, 7, max_paths=768)
    _equal(rgba, colors, orgba, ocol, f"cornell_box_path {knob}")
    assert st["batches"] >= 3
    if knob[0] == "JSRT_BOUND_MARGIN":
        assert st["attempts"] >= 2  # a level outgrew its halved bound: LVL_UNDER, the frame redone
