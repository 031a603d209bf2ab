"""The SDF zoo (tests/golden/sdfzoo, oracle/refharness/zoo_scenes.js + regen_zoo.sh): scenes whose SDF trees lie outside
the shapes of the reference's seven SDF scenes -- RoundSDF, n-ary Union / Intersection of mixed children, nested
TransformSDF, Sequences mixing Matrix / Reflection / Repetition (sizes that are no powers of two), nested and
zero-iteration loops, smooth combinators nested to the blend stack's depth, a scene mixing a form root with VM roots
and an SDF primitive inside an Aggregate -- with every known answer computed by the reference itself.

Here, without a GPU:
  * the oracle against those answers: World.cast (t as u64 bits, obj), material_data (normal, position, uv[:2], bary,
    basecolor bit for bit on hits, NaN = absent, as tests/test_gpu_material.py), SDF.distance bit for bit, the render
    (RGBA8 exact, the same NaN/inf pattern, |dRGB| <= 1e-5: tests/test_gpu_parity.py's bar);
  * the native JSON reader: blob_from_json(Serializer JSON) is the exported blob byte for byte;
  * what the loader decided (jsrt_sdf_forms, host-only): every zoo root but zoo_mixed's sponge is form 0 (the program
    VM), the seven reference scenes are forms, and are form 0 under JSRT_SDF_NOFORMS=1 -- so a matcher that one day
    swallows a zoo shape cannot silently move these tests off the VM;
  * at least a quarter of each scene's primary rays hit an SDF primitive whose root runs the VM (a scene must not
    pass by missing), and the eight-deep smooth chain's hits are blends, each its own colour;
  * the program limits (sdf_program.h): the zoo trees sit at SDF_MAX_D / _P / _S / _LOOP and SDF_MAX_BLEND and load;
    trees one past each, made by editing the zoo JSON, are refused by the loader, whose message names that stack alone."""
import copy
import json

import numpy as np
import pytest

from oracle import pyoracle

SUB = "sdfzoo"
ZOO = pyoracle.golden_cast_scenes(SUB)
RENDERS = pyoracle.golden_index(SUB)
REFERENCE_SDF = ["SDF_BoxBall", "SDF_Combinations", "SDF_Menger", "SDF_RecursiveUnionTest", "SDF_Sierpinski", "SDF_Simple",
                 "SDF_SphereRepetition"]
TOL = 1e-5
SFORM_RUNION_DIFF = 1  # sdf_program.h
# OBJS index -> root form of every SDFGeometry primitive (object 0 is the floor)
ZOO_FORMS = {
    "zoo_round_nary": {1: 0},
    "zoo_union_wide": {1: 0},
    "zoo_nested_tx": {1: 0},
    "zoo_loops": {1: 0, 2: 0, 3: 0},
    "zoo_smooth_chain": {1: 0, 2: 0},
    "zoo_mixed": {1: SFORM_RUNION_DIFF, 2: 0, 3: 0, 5: 0},  # 4: the analytic sphere, 5: the Aggregate's child, 6: the Aggregate
}


@pytest.fixture(scope="module")
def jr():
    import jsraytracer_amd as jr
    return jr


def test_zoo_is_complete():
    assert ZOO == sorted(ZOO_FORMS) == pyoracle.golden_material_scenes(SUB)
    assert sorted({r["scene"] for r in RENDERS.values()}) == ZOO
    for r in RENDERS.values():  # partial 8 x 8 patches in both directions
        assert (r["width"], r["height"], r["depth"]) == (28, 20, 4)


def _diff_rows(a, b):
    """rows where the f32 bit patterns differ (NaN == NaN: absent on both sides)."""
    same = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    return np.flatnonzero(~same.all(1))


@pytest.mark.parametrize("name", ZOO)
def test_oracle_cast_matches_reference(name):
    blob = pyoracle.golden_scene(name, SUB)
    for s in pyoracle.golden_casts(name, SUB)["sets"]:
        t, obj = pyoracle.cast(blob, s["rays"], s["minD"], s["maxD"], s["transp"])
        bad = np.flatnonzero((obj != s["obj"]) | (t.view(np.uint64) != s["t"].view(np.uint64)))
        assert bad.size == 0, (f"{name}.{s['name']}: {bad.size} of {len(t)} differ, first ray {bad[0]} {s['rays'][bad[0]]}: "
                               f"{t[bad[0]]!r} obj {obj[bad[0]]} vs {s['t'][bad[0]]!r} obj {s['obj'][bad[0]]}")


@pytest.mark.parametrize("name", ZOO)
def test_primary_rays_hit_sdf(name):
    prim = pyoracle.golden_casts(name, SUB)["sets"][0]
    assert prim["name"] == "primary" and prim["n"] == 28 * 20
    share = np.isin(prim["obj"], list(ZOO_FORMS[name])).mean()
    vm = np.isin(prim["obj"], [o for o, form in ZOO_FORMS[name].items() if form == 0]).mean()
    print(f"{name}: {share:.3f} of the primary rays hit an SDF primitive, {vm:.3f} one whose root runs the VM")
    assert vm >= 0.25  # the form root of zoo_mixed does not count: the scenes are here for the VM


def test_smooth_chain_hits_are_blends():
    """The eight-deep chain's known answers must depend on the blends below the root: a hit whose mix factor is 0 or
    1 at some level carries one operand's data and says nothing of the other's pending blend.  At least half of the
    chain primitive's hits (a majority; the scene is built so that nearly all do) carry a basecolour that is no
    leaf's, and no two of those hits the same one."""
    leaves = {tuple(np.float32(d["_v"]["basecolor"]["_v"])) for d in _walk(_geometry(_doc("zoo_smooth_chain"), 0)["root_sdf"])
              if isinstance(d.get("_v"), dict) and "basecolor" in d["_v"]}
    assert len(leaves) == 9  # the innermost leaf and each level's second operand
    m = pyoracle.golden_material("zoo_smooth_chain", SUB)["material"]
    bc = m["basecolor"][m["obj"] == 1]
    blended = np.array([tuple(c) not in leaves for c in bc])
    print(f"zoo_smooth_chain: {int(blended.sum())} of {len(bc)} hits on the chain are blends")
    assert len(bc) >= 100 and blended.mean() >= 0.5
    assert len(np.unique(bc[blended], axis=0)) >= 0.9 * blended.sum()


@pytest.mark.parametrize("name", ZOO)
def test_oracle_material_data_matches_reference(name):
    m = pyoracle.golden_material(name, SUB)["material"]
    got = pyoracle.material_data(pyoracle.golden_scene(name, SUB), m["rays"])
    assert np.array_equal(got["obj"], m["obj"])
    assert np.array_equal(got["t"].view(np.uint64), m["t"].view(np.uint64))
    hit = m["obj"] >= 0
    for f, cols in (("normal", 4), ("position", 4), ("uv", 2), ("bary", 3), ("basecolor", 3)):
        bad = _diff_rows(got[f][hit, :cols], m[f][hit, :cols])
        assert bad.size == 0, (f"{name}.{f}: {bad.size} of {int(hit.sum())} hits differ, first: ray {m['rays'][hit][bad[0]]} "
                               f"{got[f][hit][bad[0]]} vs {m[f][hit][bad[0]]}")


@pytest.mark.parametrize("name", ZOO)
def test_oracle_sdf_distance_matches_reference(name):
    kat = pyoracle.golden_material(name, SUB)
    assert sorted(e["obj"] for e in kat["sdf"]) == sorted(ZOO_FORMS[name])
    blob = pyoracle.golden_scene(name, SUB)
    for e in kat["sdf"]:
        d = pyoracle.sdf_distance(blob, e["obj"], e["points"])
        bad = np.flatnonzero(d.view(np.uint64) != e["distance"].view(np.uint64))
        assert bad.size == 0, (f"{name} obj {e['obj']}: {bad.size} of {len(d)} differ, first at {e['points'][bad[0]]}: "
                               f"{d[bad[0]]!r} vs {e['distance'][bad[0]]!r}")


def compare_render(rgba, colors, grgba, gcol, label):
    bad = (rgba != grgba).any(-1)
    assert not bad.any(), f"{label}: {int(bad.sum())} RGBA8 pixels differ"
    fin = np.isfinite(gcol[..., :3])
    assert np.array_equal(np.isfinite(colors[..., :3]), fin), f"{label}: NaN/inf pattern differs"
    err = float(np.abs(colors[..., :3][fin] - gcol[..., :3][fin]).max()) if fin.any() else 0.0
    assert err <= TOL, f"{label}: max |dRGB| {err}"


@pytest.mark.parametrize("tag", sorted(RENDERS))
def test_oracle_render_matches_reference(tag):
    r = RENDERS[tag]
    gcol, grgba = pyoracle.golden_image(tag, r["width"], r["height"], SUB)
    ocol, orgba, st = pyoracle.render(pyoracle.golden_scene(r["scene"], SUB), r["width"], r["height"], r["spp"], r["depth"],
                                      r["kind"], r["seed"])
    compare_render(orgba, ocol, grgba, gcol, tag)
    assert st["draws"] == r["draws"] and st["color_calls"] == r["color_calls"]


@pytest.mark.parametrize("name", ZOO)
def test_json_reader_reproduces_blob(jr, name):
    blob, _ = jr.blob_from_json(pyoracle.golden_json(name, SUB))
    assert blob == pyoracle.golden_scene(name, SUB)


# ---- what the loader decided ----
@pytest.mark.parametrize("name", ZOO)
def test_zoo_roots_run_the_vm(jr, name):
    f = jr.sdf_forms(pyoracle.golden_scene(name, SUB))
    print(f"{name}: {f}")
    assert f == {"all_forms": 0, "roots": ZOO_FORMS[name]}


@pytest.mark.parametrize("name", REFERENCE_SDF)
def test_reference_scenes_are_forms(jr, monkeypatch, name):
    blob = pyoracle.golden_scene(name)
    f = jr.sdf_forms(blob)
    assert f["all_forms"] == 1 and f["roots"] and all(v > 0 for v in f["roots"].values()), f
    monkeypatch.setenv("JSRT_SDF_NOFORMS", "1")
    g = jr.sdf_forms(blob)
    assert g == {"all_forms": 0, "roots": {k: 0 for k in f["roots"]}}


# ---- limits: edits of the zoo JSON (the reference's Serializer format: {"_t": type, "_v": value}, a type written
# ["Name", id] where the document first uses it and id afterwards; "_r" marks and references shared objects) ----
def _walk(x):
    if isinstance(x, dict):
        yield x
        for v in x.values():
            yield from _walk(v)
    elif isinstance(x, list):
        for v in x:
            yield from _walk(v)


def _type_id(doc, name):
    for d in _walk(doc):
        if isinstance(d.get("_t"), list) and d["_t"][0] == name:
            return d["_t"][1]
    raise KeyError(name)


def _is(doc, node, name):
    t = node.get("_t")
    return (t[1] if isinstance(t, list) else t) == _type_id(doc, name)


def _clone(node):
    """A copy that defines no shared object again: a node's own "_r" mark goes, pure references stay."""
    c = copy.deepcopy(node)
    for d in _walk(c):
        if "_v" in d:
            d.pop("_r", None)
    return c


def _finish(doc):
    """Type names back where the document first uses each type, then the text."""
    names = {d["_t"][1]: d["_t"][0] for d in _walk(doc) if isinstance(d.get("_t"), list)}
    seen = set()
    for d in _walk(doc):
        if "_t" in d:
            i = d["_t"][1] if isinstance(d["_t"], list) else d["_t"]
            d["_t"] = i if i in seen else [names[i], i]
            seen.add(i)
    return json.dumps(doc)


def _doc(name):
    return json.loads(pyoracle.golden_json(name, SUB))


def _geometry(doc, k):
    """The k-th SDFGeometry of the document: the dict whose "root_sdf" is its tree."""
    return [d["_v"] for d in _walk(doc) if isinstance(d.get("_v"), dict) and "root_sdf" in d["_v"]][k]


def _node(doc, name, value):
    return {"_t": _type_id(doc, name), "_v": dict({"UID": 100000}, **value)}


def _array(doc, items):
    return {"_t": _type_id(doc, "Array"), "_v": items}


def _seventh_union_child():  # SDF_MAX_D: seven distances at the root's Math.min
    doc = _doc("zoo_union_wide")
    kids = _geometry(doc, 0)["root_sdf"]["_v"]["children"]["_v"]
    assert len(kids) == 6
    kids.append(_clone(kids[-1]))
    return doc


def _third_nested_transform():  # SDF_MAX_P: Transform(Transform(Transform(Sphere, M), M), M), scale stack 3 (allowed)
    doc = _doc("zoo_round_nary")
    outer = _geometry(doc, 0)["root_sdf"]["_v"]["child_sdf"]["_v"]["children"]["_v"][1]
    assert _is(doc, outer, "TransformSDF") and _is(doc, outer["_v"]["child_sdf"], "SphereSDF")
    m = outer["_v"]["transformer"]
    assert _is(doc, m, "SDFMatrixTransformer")
    for _ in range(2):
        outer["_v"]["child_sdf"] = _node(doc, "TransformSDF", {"child_sdf": outer["_v"]["child_sdf"], "transformer": _clone(m)})
    return doc


def _fifth_scale_level():  # SDF_MAX_S: Sequence(Sequence(Sequence(Matrix)), ...) under two TransformSDFs
    doc = _doc("zoo_nested_tx")
    seq = _geometry(doc, 0)["root_sdf"]["_v"]["child_sdf"]["_v"]["transformer"]
    items = seq["_v"]["transformers"]["_v"]
    assert _is(doc, seq, "SDFTransformerSequence") and _is(doc, items[0], "SDFTransformerSequence")
    items[0] = _node(doc, "SDFTransformerSequence", {"transformers": _array(doc, [items[0]])})
    return doc


def _sequence_around_the_recursive():  # SDF_MAX_S again: RecursiveTransformUnion(Sphere, Sequence(Recursive(Sequence(..))))
    doc = _doc("zoo_loops")
    root = _geometry(doc, 0)["root_sdf"]
    assert _is(doc, root, "RecursiveTransformUnionSDF") and _is(doc, root["_v"]["transformer"], "SDFRecursiveTransformer")
    root["_v"]["transformer"] = _node(doc, "SDFTransformerSequence", {"transformers": _array(doc, [root["_v"]["transformer"]])})
    return doc


def _third_nested_loop():  # SDF_MAX_LOOP: Recursive(Recursive(Matrix, 1), 2) in a union loop (scale stack: 4, allowed)
    doc = _doc("zoo_loops")
    rec = _geometry(doc, 0)["root_sdf"]["_v"]["transformer"]
    step = rec["_v"]["transformer"]
    assert _is(doc, step, "SDFTransformerSequence")
    matrix = step["_v"]["transformers"]["_v"][0]
    assert _is(doc, matrix, "SDFMatrixTransformer")
    rec["_v"]["transformer"] = _node(doc, "SDFRecursiveTransformer", {"transformer": matrix, "iterations": 1})
    return doc


def ninth_smooth_level():  # SDF_MAX_BLEND: one more smooth combinator around zoo_smooth_chain's eight
    doc = _doc("zoo_smooth_chain")
    g = _geometry(doc, 0)
    root, depth, n = g["root_sdf"], 0, g["root_sdf"]
    while "childA" in n["_v"] or "positive" in n["_v"]:
        n, depth = n["_v"].get("childA", n["_v"].get("positive")), depth + 1
    assert depth == 8 and _is(doc, root, "SmoothUnionSDF")
    g["root_sdf"] = _node(doc, "SmoothUnionSDF", {"k": 0.3, "childA": root, "childB": _clone(root["_v"]["childB"])})
    return _finish(doc)


# each edit with the one stack it overflows, as the loader's message names it
ONE_PAST = [(_seventh_union_child, "distance stack 7 > 6"), (_third_nested_transform, "point stack 3 > 2"),
            (_fifth_scale_level, "scale stack 5 > 4"), (_sequence_around_the_recursive, "scale stack 5 > 4"),
            (_third_nested_loop, "loop nesting 3 > 2")]


@pytest.mark.parametrize("name", ZOO)
def test_json_edit_helpers_keep_the_scene(jr, name):
    """_finish on an untouched document gives the exported blob (the edits below change the trees, nothing else)."""
    assert jr.blob_from_json(_finish(_doc(name)))[0] == pyoracle.golden_scene(name, SUB)


@pytest.mark.parametrize("edit,over", ONE_PAST, ids=[e.__name__.strip("_") for e, _ in ONE_PAST])
def test_tree_one_past_a_stack_limit_is_refused(jr, edit, over):
    """Refused with "too deep/wide", and for that stack alone: the message ends with the one overflow."""
    blob, _ = jr.blob_from_json(_finish(edit()))
    with pytest.raises(jr.JsrtError, match=f"too deep/wide for the GPU program stacks: {over}$"):
        jr.sdf_forms(blob)


def test_ninth_nested_smooth_combinator_is_refused(jr):
    """The reference blends getMaterialData through any depth; the device keeps SDF_MAX_BLEND = 8 pending blends
    (device_common.h sdf_material), so the loader refuses the ninth level instead of letting the walk stop early
    (zoo_smooth_chain's eight levels load and match the reference bit for bit)."""
    blob, _ = jr.blob_from_json(ninth_smooth_level())
    with pytest.raises(jr.JsrtError, match="nested 9 deep: the GPU blend stack holds 8"):
        jr.sdf_forms(blob)
