"""The light samples per lit node (ns: the sum over the lights, a point light counting 1) decide W.group, the
k_shadow form and the bucketed or unbucketed hand-off (render.hip render_frame, render_levels.h run_batch), and
scale max_paths in plan_batches.  The committed scenes hold only ns = 4 (cornell's Square light), 1 (heart's Sphere
light) and point lights; here the `samples` of a light record of the committed Serializer JSON
(tests/golden/json, _v.renderer._v.world._v.lights._v[i]._v.samples) is edited, the JSON re-encoded and read by
jr.blob_from_json, and that one blob rendered by the oracle and by the GPU.  Bar (test_gpu_parity): RGBA8
identical, the same NaN/inf pattern, |dRGB| <= 1e-5, stats["samples"] exact; a knob variant also equals the
default render of a fresh Scene bit for bit (rgba and the u32 view of colors).

The arm each case is meant to reach (kernel instantiation, group, hand-off):
cornell_box_path (PF_ANALYTIC, hybrid chain run_batch<PF_ANALYTIC,true>, Square light, staged tables):
  1    k_shadow<PF_ANALYTIC,true,false,false,true>, group 1, grid-cell buckets (ns = 1 is not a k_shadow_node case)
  2    k_shadow_node<PF_ANALYTIC,true,4>, two of four samples (JSRT_SHADOW_NODE=1 / default); =0: k_shadow group 2
  3    k_shadow_node<...,4> with a short last sample; JSRT_SHADOW_NODE=0: k_shadow group 4, one idle lane;
       JSRT_BUCKET=0: k_shadow group 4 unbucketed (INFO_LIT from the node, chain_slot); JSRT_HYBRID=0: the tree,
       run_batch<PF_ANALYTIC,false>: k_shade<PF_ANALYTIC,false,true>, k_shadow_node<PF_ANALYTIC,false,4>
  5    k_shadow<...,false,false,true> group 8, 3 idle lanes, bucketed
  8    group 8 full; JSRT_BUCKET=0 unbucketed; max_paths=640: several batches, partly filled last blocks
  33   group 64, 31 idle lanes        64   group 64: one full wave per node
  65   k_shadow<PF_ANALYTIC,true,true,false,false> (SERIAL, group 1), W.bucket off (ns > 64); JSRT_HYBRID=0:
       k_shadow<PF_ANALYTIC,false,true,false,false>; max_paths=640: plan_batches' 640 * 4 / 65 = 39 -> floor of 64
  100  SERIAL, the rescale at the default max_paths
cornell_box (Phong walls, ambient 0.1):  3  k_shadow_node over a non-zero ambient;  7  k_shadow group 8
heart (PF_MESH, tree, Sphere light: SPH = true, primitive buckets):
  2, 4, 7  k_shadow<PF_MESH,false,false,true,false> group 2 / 4 / 8 (SPH with group > 1; 7: an idle lane)
  4 + JSRT_SHADOW_SERIAL=1  k_shadow<PF_MESH,false,true,true,false>, bucketed
  70   k_shadow<PF_MESH,false,true,true,false>, unbucketed (ns > 64)
cornell_box_path + refraction_path's first point light (n_lights = 2, so never k_shadow_node):
  area 3 (ns = 4)  k_shadow<PF_ANALYTIC,true,false,false,true> group 4 under both JSRT_SHADOW_NODE settings
  area 6 (ns = 7)  group 8, one idle lane, the point light on the last used lane
SDF_Simple + cornell_box_path's area light (PF_SDF, persistent casts: k_extend_q<PF_SDF,...>):
  area 3 (ns = 4)  k_shadow_prep / k_shadow_cast / k_shadow_sum with group 4
  area 70 (ns = 71) k_shadow<PF_SDF,false,true,false,false> (serial) beside the persistent extends, unbucketed
  both also with JSRT_HYBRID=1 (the CHAIN = true instantiations); area 3 also with JSRT_PERSIST=0: bucketed
  k_shadow<PF_SDF,false,false,false,false> group 4
heart 70 also with JSRT_HYBRID=1 (the serial Sphere-light k_shadow on the schedule the knob selects)

A light record of the Serializer is not self-contained: `_t` is [class name, id] where a class first appears in
the document and the bare id afterwards, the ids being the document's own.  The transplanted record (the last two
groups) is copied with every `_t` rewritten to its [name, id] form, the id being the receiving document's for that
class name or a fresh one; it holds no `_r` reference (asserted).  Nothing else of it is touched."""
import gzip
import json
import os

import numpy as np
import pytest

from oracle import pyoracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JDIR = os.path.join(ROOT, "tests", "golden", "json")
SIDE = {"heart": os.path.join(JDIR, "heart.obj.gz")}  # (test_gpu_json.py's side files)
TOL = 1e-5
NODE0, NODE1 = {"JSRT_SHADOW_NODE": "0"}, {"JSRT_SHADOW_NODE": "1"}


def _gz(p):
    with gzip.open(p, "rb") as f:
        return f.read()


def _doc(scene):
    return json.loads(_gz(os.path.join(JDIR, scene + ".json.gz")))


def _lights(doc):
    return doc["_v"]["renderer"]["_v"]["world"]["_v"]["lights"]["_v"]


def _walk(x):
    if isinstance(x, dict):
        yield x
        for v in x.values():
            yield from _walk(v)
    elif isinstance(x, list):
        for v in x:
            yield from _walk(v)


def _types(doc):
    """class id -> name of a Serializer document"""
    return {o["_t"][1]: o["_t"][0] for o in _walk(doc) if isinstance(o.get("_t"), list)}


def _transplant(record, src, dst):
    """A copy of src's `record` for dst's document: every _t as [name, dst's id of that name or a fresh one]."""
    names, ids = _types(src), {n: i for i, n in _types(dst).items()}
    rec = json.loads(json.dumps(record))
    for o in _walk(rec):
        assert "_r" not in o, "a shared reference inside the light record"
        if "_t" in o:
            t = o["_t"]
            name = t[0] if isinstance(t, list) else names[t]
            if name not in ids:
                ids[name] = max(ids.values()) + 1
            o["_t"] = [name, ids[name]]
    return rec


def _with_samples(scene, samples):
    doc = _doc(scene)
    (area,) = [l for l in _lights(doc) if "samples" in l["_v"]]
    area["_v"]["samples"] = samples
    return doc


def _cornell_and_point(samples):
    doc = _with_samples("cornell_box_path", samples)
    src = _doc("refraction_path")
    _lights(doc).append(_transplant(_lights(src)[0], src, doc))
    return doc


def _sdf_and_area(samples):
    doc, src = _doc("SDF_Simple"), _with_samples("cornell_box_path", samples)
    _lights(doc).append(_transplant(_lights(src)[0], src, doc))
    return doc


SCENES = {"cornell_box_path": lambda n: _with_samples("cornell_box_path", n),
          "cornell_box": lambda n: _with_samples("cornell_box", n),
          "heart": lambda n: _with_samples("heart", n),
          "cornell_point": _cornell_and_point,
          "sdf_area": _sdf_and_area}

S, L = (28, 20), (44, 36)
# (scene, samples, (W, H), spp, depth cap, seed, [(render kwargs, environment) variants beside the default render])
CASES = [
    ("cornell_box_path", 1, S, 3, 6, 11, []),
    ("cornell_box_path", 2, L, 2, 6, 12, [({}, NODE0), ({}, NODE1)]),
    ("cornell_box_path", 3, L, 5, 6, 13, [({}, NODE0), ({}, NODE1), ({}, {"JSRT_BUCKET": "0"}), ({}, {"JSRT_HYBRID": "0"})]),
    ("cornell_box_path", 5, S, 4, 6, 14, []),
    ("cornell_box_path", 8, L, 3, 6, 15, [({}, {"JSRT_BUCKET": "0"}), ({"max_paths": 640}, {})]),
    ("cornell_box_path", 33, S, 2, 6, 16, []),
    ("cornell_box_path", 64, S, 3, 6, 17, []),
    ("cornell_box_path", 65, S, 5, 6, 18, [({}, {"JSRT_HYBRID": "0"}), ({"max_paths": 640}, {})]),
    ("cornell_box_path", 100, S, 3, 6, 19, []),
    ("cornell_box", 3, L, 3, 6, 21, []),
    ("cornell_box", 7, S, 2, 6, 22, []),
    ("heart", 2, S, 3, 4, 31, []),
    ("heart", 4, L, 2, 4, 32, [({}, {"JSRT_SHADOW_SERIAL": "1"})]),
    ("heart", 7, S, 5, 4, 33, []),
    ("heart", 70, S, 2, 4, 34, [({}, {"JSRT_HYBRID": "1"})]),
    ("cornell_point", 3, L, 3, 6, 41, [({}, NODE0), ({}, NODE1)]),
    ("cornell_point", 6, S, 2, 6, 42, []),
    ("sdf_area", 3, L, 3, 4, 51, [({}, {"JSRT_HYBRID": "1"}), ({}, {"JSRT_PERSIST": "0"})]),
    ("sdf_area", 70, S, 2, 4, 52, [({}, {"JSRT_HYBRID": "1"})]),
]


def _id(c):
    return f"{c[0]}_n{c[1]}_{c[2][0]}x{c[2][1]}_s{c[3]}"


@pytest.fixture(scope="module")
def jr():
    import jsraytracer_amd as jr
    return jr


_blobs, _oracle = {}, {}


def _blob(jr, scene, samples):
    if (scene, samples) not in _blobs:
        side = [_gz(SIDE[scene])] if scene in SIDE else []
        _blobs[scene, samples] = jr.blob_from_json(json.dumps(SCENES[scene](samples)), side)[0]
    return _blobs[scene, samples]


def _reference(blob, name, W, H, spp, depth, seed):
    key = (name, W, H, spp, depth, seed)
    if key not in _oracle:
        ocol, orgba, _ = pyoracle.render(blob, W, H, spp, depth, 1, seed)
        ocol.setflags(write=False)
        orgba.setflags(write=False)
        _oracle[key] = (ocol, orgba)
    return _oracle[key]


def _compare(rgba, colors, grgba, gcol, label):
    bad = (rgba != grgba).any(-1)
    assert not bad.any(), f"{label}: {int(bad.sum())} RGBA8 pixels differ"
    fin = np.isfinite(gcol[..., :3])
    assert np.array_equal(np.isfinite(colors[..., :3]), fin), f"{label}: NaN/inf pattern differs"
    err = float(np.abs(colors[..., :3][fin] - gcol[..., :3][fin]).max()) if fin.any() else 0.0
    assert err <= TOL, f"{label}: max |dRGB| {err}"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_light_sample_counts_match_oracle(jr, monkeypatch, case):
    scene, samples, (W, H), spp, cap, seed, variants = case
    blob = _blob(jr, scene, samples)
    depth = min(cap, pyoracle.scene_header(blob)["max_depth"])
    ocol, orgba = _reference(blob, f"{scene}:{samples}", W, H, spp, depth, seed)
    assert int((orgba[..., :3] > 0).any(-1).sum()) > W * H // 8  # a lit image, not a black one
    rgba0, col0, st = jr.Scene(blob, device=0).render(W, H, spp, depth, 1, seed)
    _compare(rgba0, col0, orgba, ocol, _id(case))
    assert st["samples"] == W * H * spp
    for kw, env in variants:
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            rgba, colors, st = jr.Scene(blob, device=0).render(W, H, spp, depth, 1, seed, **kw)
        label = f"{_id(case)} {kw} {env}"
        _compare(rgba, colors, orgba, ocol, label)
        assert st["samples"] == W * H * spp, label
        assert np.array_equal(rgba, rgba0), label
        assert np.array_equal(colors.view(np.uint32), col0.view(np.uint32)), label
        if kw.get("max_paths"):
            assert st["batches"] >= 3, label
