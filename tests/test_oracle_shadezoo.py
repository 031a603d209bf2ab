"""The shading zoo (tests/golden/shadezoo, oracle/refharness/shade_zoo_scenes.js + regen_shadezoo.sh): scenes of this
project's own, built from the reference's classes, that construct the materials and lights the loader accepts and the
kernels implement but no reference scene uses -- with every known answer computed by the reference itself.

Which scene reaches which branch, and the assertion that fails if the branch is skipped or computed differently
(objects by OBJS index, as shade_zoo_scenes.js lists them; "render" = test_oracle_render_matches_reference here and
test_gpu_shadezoo_render_matches_reference on the device, together with the reach test named):
  * SolidColorMaterial, TransparentMaterial (shade_node's early returns; the unnormalised-direction child of weight
    1 - opacity, an unlit node alone or next to lit ones): shz_solid_transparent objects 1-9 -- Solid with a solid and
    a checkerboard colour, Transparent at 0.35 / 0 / 1, one that casts no shadow, four sheets in a row under depth 4,
    beside object 10 (Phong transmissivity: the normalised direction).  test_targets_are_hit + render;
    test_shadow_sets_are_mixed for the primitive that casts no shadow.
  * Circle area lights: shz_light_mix light 0 (rotation x non-uniform scale, samples 3), shz_profiles_* light 0.
    render; test_circle_light_samples_like_square (see there: what a Circle changes is its bounding box alone, which
    no colour depends on, so the edit Circle -> Square must leave the reference's image as it is).
  * A light colour that reads UV: shz_light_uv -- point light (cartesianToSpherical of the direction), Sphere light
    (UV of the picked normal), rotated Square light (local xy) whose checkerboard sits in a ScaledMaterialColor.
    test_light_edit_changes_the_image[checker_*] + render.  The reference's spherical UV lies in [0, 1]^2, where the
    checkerboard is its first colour: for the point and the Sphere light the known answer pins that the device's UV
    stays in that square (the second colours are far from the first), and swapping the two colours changes the image.
  * Transformed Sphere lights: shz_light_uv light 1 (rotation x non-uniform scale: the inv_transform.transposed()
    normal), shz_light_mix light 2 (a Sphere light between other area lights: staggered sample_call offsets).
    test_light_edit_changes_the_image[sphere_translation_only] + render.
  * PhongMaterial with reflectivity and transmissivity: shz_phong_children objects 2 (two children), 3 (vector
    reflectivity), 4 (per-channel scaled reflectivity and transmissivity), 1 (checkerboard reflectivity with a black
    colour: one or two children by the hit's UV).  test_targets_are_hit, test_checker_reflectivity_hits_both + render.
  * Fresnel edges: shz_fresnel_edges objects 1 (ratio 0.75), 2 (ratio 1: kr == 0), 3 (1.5, a point light inside),
    4 (Infinity), 5 (a ratio-1.5 pane seen from its backside).  test_fresnel_branch_counts + render.
  * PhongPathTracingMaterial scatter: shz_path_scatter objects 1 (mirror 0.3, ratio Infinity), 2 (mirror 0.5, ratio
    1.5), 3 and 5 (probSum == 0), 4 (specular only).  test_targets_are_hit + render (draws and color_calls exact:
    a scatter that draws once more or less, or spawns a child it should not, moves both).
  * Specular exponent edges: shz_phong_children objects 5 (smoothness 0: Math.pow(0, 0)), 6 (smoothness 1e6 with
    specularity 0, outside MATF_SPEC_ZERO's bound), 7 (specularity 0 with ambient).  test_targets_are_hit + render.
  * Other profiles: the Solid, Transparent, two-child Phong and Fresnel 0.75 materials on SDFGeometry primitives alone
    (shz_profiles_sdf objects 1-4: the SDF profile), on the triangles of a BVH built as the reference's hollow
    tetrahedron scene builds one (shz_profiles_mesh 1-4: the mesh profile), and inside an Aggregate beside an SDF
    primitive and a BVH (shz_profiles_all 1-4, 6, 7-8: every feature at once), each under a Circle light.
    test_targets_are_hit + render.

Here, without a GPU: the oracle against the reference's answers (casts, material_data, renders with draws and
color_calls), the native JSON reader against the exported blob, the reach conditions above from the fixtures alone,
the fixture sizes, and the sensitivity of the goldens to the light-side features."""
import json
import os
import struct

import numpy as np
import pytest

from oracle import pyoracle
from test_oracle_sdfzoo import _diff_rows, _finish, _is, _type_id, _walk, compare_render

SUB = "shadezoo"
ZOO = pyoracle.golden_cast_scenes(SUB)
RENDERS = pyoracle.golden_index(SUB)
DEPTH = {"shz_solid_transparent": 4, "shz_phong_children": 5, "shz_fresnel_edges": 6, "shz_path_scatter": 5,
         "shz_light_uv": 4, "shz_light_mix": 4, "shz_profiles_sdf": 5, "shz_profiles_mesh": 5, "shz_profiles_all": 5}
PATH_SCENES = ["shz_path_scatter"]
LIGHT_SCENES = ["shz_light_uv", "shz_light_mix"]
# the primitives that carry a targeted material (shz_solid_transparent's sheets 7-9 stand behind sheet 6: they are
# reached by its children only, and the depth-4 renders pin them); the light scenes' targets are their lights
TARGETS = {
    "shz_solid_transparent": [1, 2, 3, 4, 5, 6, 10],
    "shz_phong_children": [1, 2, 3, 4, 5, 6, 7],
    "shz_fresnel_edges": [1, 2, 3, 4, 5],
    "shz_path_scatter": [1, 2, 3, 4, 5],
    "shz_light_uv": [],
    "shz_light_mix": [2],
    "shz_profiles_sdf": [1, 2, 3, 4],
    "shz_profiles_mesh": [1, 2, 3, 4],
    "shz_profiles_all": [1, 2, 3, 4, 6, 7, 8],
}
NO_SHADOW = {"shz_solid_transparent": 4, "shz_light_mix": 2}  # the primitive with does_cast_shadow false
FRESNEL_RATIO = {1: 0.75, 2: 1.0, 3: 1.5, 5: 1.5}  # shz_fresnel_edges, the finite ratios
INSIDE_LIGHT = np.array([0.2, 0.15, 1.1])  # shz_fresnel_edges light 1, inside object 3


@pytest.fixture(scope="module")
def jr():
    import jsraytracer_amd as jr
    return jr


def _doc(name):
    return json.loads(pyoracle.golden_json(name, SUB))


def test_zoo_is_complete():
    assert ZOO == sorted(DEPTH) == pyoracle.golden_material_scenes(SUB)
    assert sorted({r["scene"] for r in RENDERS.values()}) == ZOO
    for name in ZOO:
        rs = sorted((r["kind"], r["spp"]) for r in RENDERS.values() if r["scene"] == name)
        assert rs == ([(1, 3), (2, 2)] if name in PATH_SCENES else [(0, 1), (1, 2)]), name
    for r in RENDERS.values():  # partial 8 x 8 patches in both directions
        assert (r["width"], r["height"], r["depth"]) == (28, 20, DEPTH[r["scene"]]) and r["depth"] <= 6


def test_fixture_sizes():
    """No file larger than the largest of its kind in the SDF zoo, whose layout this tree shares."""
    for kind in ("scenes", "images", "casts", "material", "json"):
        def largest(sub):
            d = os.path.join(pyoracle.GOLDEN, sub, kind)
            return max(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))
        assert largest(SUB) <= largest("sdfzoo"), kind
    assert os.path.getsize(os.path.join(pyoracle.GOLDEN, SUB, "index.json")) <= 1 << 20


# ---- the oracle against the reference's answers ----
@pytest.mark.parametrize("name", ZOO)
def test_oracle_cast_matches_reference(name):
    blob = pyoracle.golden_scene(name, SUB)
    sets = pyoracle.golden_casts(name, SUB)["sets"]
    assert [(s["name"], s["n"]) for s in sets] == [("primary", 28 * 20), ("random", 256), ("shadow", 256)]
    for s in sets:
        t, obj = pyoracle.cast(blob, s["rays"], s["minD"], s["maxD"], s["transp"])
        bad = np.flatnonzero((obj != s["obj"]) | (t.view(np.uint64) != s["t"].view(np.uint64)))
        assert bad.size == 0, (f"{name}.{s['name']}: {bad.size} of {len(t)} differ, first ray {bad[0]} {s['rays'][bad[0]]}: "
                               f"{t[bad[0]]!r} obj {obj[bad[0]]} vs {s['t'][bad[0]]!r} obj {s['obj'][bad[0]]}")


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


# ---- reach: from the fixtures alone, so a scene cannot pass by missing its target ----
def _primary(name):
    """The primary rays' rows of the material KAT (the first 28 x 20 of its rays) as f64."""
    m = pyoracle.golden_material(name, SUB)["material"]
    prim = pyoracle.golden_casts(name, SUB)["sets"][0]
    n = prim["n"]
    assert prim["name"] == "primary" and np.array_equal(m["rays"][:n], prim["rays"]) and np.array_equal(m["obj"][:n], prim["obj"])
    return {k: np.asarray(v[:n], np.float64 if v.dtype.kind == "f" else v.dtype) for k, v in m.items() if isinstance(v, np.ndarray)}


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


@pytest.mark.parametrize("name", ZOO)
def test_targets_are_hit(name):
    obj = pyoracle.golden_casts(name, SUB)["sets"][0]["obj"]
    counts = {o: int((obj == o).sum()) for o in TARGETS[name]}
    print(f"{name}: primary hits per targeted primitive {counts}")
    assert all(c >= 20 for c in counts.values()), counts


def test_fresnel_branch_counts():
    """materials.js:366-386 on the primary hits of shz_fresnel_edges, in f64 from the KAT's normals and rays: total
    internal reflection (sint >= 1), backside hits, hits that see the inside light with ldotn <= 0, and hits of the
    ratio-1 sphere (kr == 0 exactly: both of Rs and Rp vanish)."""
    p = _primary("shz_fresnel_edges")
    hit = p["obj"] >= 0  # the rays that miss carry NaN: drop them
    p = {k: v[hit] for k, v in p.items()}
    V = -_unit(p["rays"][:, 3:6])
    N = _unit(p["normal"][:, :3])
    vdotn = (V * N).sum(1)
    backside = vdotn < 0
    cosi = np.abs(vdotn)
    ratio = np.full(len(V), np.nan)
    for o, r in FRESNEL_RATIO.items():
        ratio[p["obj"] == o] = r
    on = np.isfinite(ratio)
    ni, nt = np.where(backside, ratio, 1.0), np.where(backside, 1.0, ratio)
    sint = np.where(on, ni / np.where(on, nt, 1.0), 0.0) * np.sqrt(np.maximum(0, 1 - cosi * cosi))
    tir = on & (sint >= 1)
    back = on & backside
    inside = p["obj"] == 3
    Nf = np.where(backside[:, None], -N, N)
    ldotn = (_unit(INSIDE_LIGHT - p["position"][:, :3]) * Nf).sum(1)
    away = inside & (ldotn <= 0)
    counts = {"tir": int(tir.sum()), "tir_ratio_0.75": int((tir & (p["obj"] == 1)).sum()), "tir_backside": int((tir & back).sum()),
              "backside": int(back.sum()), "refracting_backside": int((back & ~tir).sum()),
              "ldotn<=0 to the inside light": int(away.sum()), "ratio_1": int((p["obj"] == 2).sum())}
    print(f"shz_fresnel_edges: {counts}")
    assert all(c >= 10 for c in counts.values()), counts


def test_checker_reflectivity_hits_both():
    """The wall of shz_phong_children: hits on the black squares of its reflectivity (no reflection child) and on the
    others (two children), by materials.js:73 on the KAT's UV."""
    p = _primary("shz_phong_children")
    wall = p["obj"] == 1
    u, v = p["uv"][wall, 0], p["uv"][wall, 1]
    s = np.floor(u) + np.floor(v)
    black = (s - np.floor(s / 2) * 2) % 2 >= 1
    print(f"shz_phong_children: {int(black.sum())} of {int(wall.sum())} wall hits on black squares")
    assert black.sum() >= 10 and (~black).sum() >= 10


@pytest.mark.parametrize("name", ZOO)
def test_shadow_sets_are_mixed(name):
    """Shadowed and lit segments in every scene; where a primitive casts no shadow, segments that cross it (the
    oracle's closest hit over all objects is that primitive) and that the reference leaves unshadowed."""
    s = pyoracle.golden_casts(name, SUB)["sets"][2]
    assert s["name"] == "shadow" and (s["minD"], s["maxD"], s["transp"]) == (0.0001, 1.0, False)
    shadowed = (s["t"] > 0) & (s["t"] < 1)
    print(f"{name}: {int(shadowed.sum())} of {len(shadowed)} segments shadowed")
    assert shadowed.sum() >= 20 and (~shadowed).sum() >= 20
    assert np.array_equal(s["obj"] >= 0, np.isfinite(s["t"]) & shadowed | (s["obj"] >= 0))
    if name in NO_SHADOW:
        _, through = pyoracle.cast(pyoracle.golden_scene(name, SUB), s["rays"], s["minD"], s["maxD"], True)
        crossing = through == NO_SHADOW[name]
        print(f"{name}: {int(crossing.sum())} segments cross object {NO_SHADOW[name]} first")
        assert crossing.sum() >= 3
        assert not (s["obj"] == NO_SHADOW[name]).any()
        assert (s["obj"][crossing] == -1).sum() >= 3


# ---- sensitivity: the goldens would notice a light-side feature that is dropped ----
def _lights(doc):
    return [d for d in _walk(doc) if isinstance(d.get("_v"), dict) and "color_mc" in d["_v"]]


def _checker_to_first(doc, light, swap=False):
    """The checkerboard in a light's colour chain -> its first colour (swap: its colours exchanged)."""
    holder, key = light["_v"], "color_mc"
    while not _is(doc, holder[key], "CheckerboardMaterialColor"):
        holder, key = holder[key]["_v"], "_mc"
    if swap:
        v = holder[key]["_v"]
        v["color1"], v["color2"] = v["color2"], v["color1"]
    else:
        holder[key] = holder[key]["_v"]["color1"]


def _edit_checker(k, swap=False):
    def edit():
        doc = _doc("shz_light_uv")
        _checker_to_first(doc, _lights(doc)[k], swap)
        return "shz_light_uv", doc
    return edit


def _edit_sphere_translation_only():
    doc = _doc("shz_light_uv")
    v = _lights(doc)[1]["_v"]
    assert _is(doc, v["surface_geometry"], "Sphere")
    t = [row[3] for row in v["transform"]["_v"][:3]]
    v["transform"]["_v"] = [[1, 0, 0, t[0]], [0, 1, 0, t[1]], [0, 0, 1, t[2]], [0, 0, 0, 1]]
    v["inv_transform"]["_v"] = [[1, 0, 0, -t[0]], [0, 1, 0, -t[1]], [0, 0, 1, -t[2]], [0, 0, 0, 1]]
    return "shz_light_uv", doc


def _edit_circle_to_square():
    doc = _doc("shz_light_mix")
    g = _lights(doc)[0]["_v"]["surface_geometry"]
    assert _is(doc, g, "Circle")
    g["_t"] = _type_id(doc, "Square")
    return "shz_light_mix", doc


def _render_edit(jr, edit, kind):
    """(pixels whose RGBA8 differs from the golden, the scene's name) for the oracle's render of an edited scene."""
    name, doc = edit()
    tag = next(t for t, r in sorted(RENDERS.items()) if r["scene"] == name and r["kind"] == kind)
    r = RENDERS[tag]
    blob, _ = jr.blob_from_json(_finish(doc))
    assert blob != pyoracle.golden_scene(name, SUB)
    _, rgba, _ = pyoracle.render(blob, r["width"], r["height"], r["spp"], r["depth"], r["kind"], r["seed"])
    _, grgba = pyoracle.golden_image(tag, r["width"], r["height"], SUB)
    return int((rgba != grgba).any(-1).sum())


@pytest.mark.parametrize("name", LIGHT_SCENES)
def test_json_edit_helpers_keep_the_scene(jr, name):
    assert jr.blob_from_json(_finish(_doc(name)))[0] == pyoracle.golden_scene(name, SUB)


LIGHT_EDITS = {"checker_square_to_first": _edit_checker(2), "checker_point_swapped": _edit_checker(0, True),
               "checker_sphere_swapped": _edit_checker(1, True), "sphere_translation_only": _edit_sphere_translation_only}


@pytest.mark.parametrize("edit", sorted(LIGHT_EDITS))
@pytest.mark.parametrize("kind", [0, 1], ids=["simple", "incremental"])
def test_light_edit_changes_the_image(jr, edit, kind):
    n = _render_edit(jr, LIGHT_EDITS[edit], kind)
    print(f"{edit}: {n} pixels differ from the golden")
    assert n >= 5


@pytest.mark.parametrize("k", [0, 1])
def test_spherical_light_uv_stays_on_the_first_colour(jr, k):
    """Vec.cartesianToSpherical (math.js:189-193) maps into [0, 1]^2, and floor(u) + floor(v) is 0 there but on the
    measure-zero seam: for the point light and the Sphere light the checkerboard is its first colour, so replacing it
    by that colour leaves the reference's image as it is.  What these two lights pin on the device is that its UV
    stays inside that square (their second colours are far from the first) and that the chain is evaluated
    (test_light_edit_changes_the_image[checker_*_swapped])."""
    assert _render_edit(jr, _edit_checker(k), 0) == 0


def test_circle_light_samples_like_square(jr):
    """Circle.sampleSurface and its materialData are Square's (geometry.js:295-300, 326-331, 249-254); a Circle
    differs in intersect, which no light uses, and in getBoundingBox, which no colour depends on (the device bounds a
    light by its sample domain, scene_load.cpp shadow_grid, not by the reference's box).  So no image can tell the
    two apart: the edit leaves the reference's answer unchanged, and the Circle lights are pinned by the renders."""
    assert _render_edit(jr, _edit_circle_to_square, 0) == 0
    assert _render_edit(jr, _edit_circle_to_square, 1) == 0


# ---- what cannot be reproduced is refused by name ----
def test_infinite_smoothness_scatter_is_refused(jr):
    """PhongPathTracingMaterial.scatterSpecular with an infinite smoothness calls an undefined function in the
    reference (materials.js:430): the loader names the construct instead of rendering something else."""
    doc = _doc("shz_path_scatter")
    mats = [d["_v"] for d in _walk(doc) if isinstance(d.get("_v"), dict) and "mirrorProbability" in d["_v"]]
    assert len(mats) == 6
    assert mats[1]["refractiveIndexRatio"] is None and mats[4]["smoothness"] == 40
    mats[4]["smoothness"] = None  # JSON.stringify(Infinity), as the ratio beside it
    with pytest.raises(jr.JsrtError, match="PhongPathTracingMaterial.smoothness is null"):
        jr.blob_from_json(_finish(doc))
    # the same material in the exported blob: its smoothness is the blob's one f64 of value 40
    blob = pyoracle.golden_scene("shz_path_scatter", SUB)
    forty, inf = struct.pack("<d", 40.0), struct.pack("<d", float("inf"))
    assert blob.count(forty) == 1
    jr.sdf_forms(blob)  # loads
    with pytest.raises(jr.JsrtError, match=r"infinite-smoothness path-tracing scatter is broken in the reference \(materials.js:430\)"):
        jr.sdf_forms(blob.replace(forty, inf))  # the loader, host only
