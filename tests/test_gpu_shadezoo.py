"""The HIP path on the shading zoo (tests/golden/shadezoo; tests/test_oracle_shadezoo.py describes the scenes and maps
each to the branches it reaches) -- against the reference's own known answers:
  * every render of index.json with default settings (RGBA8 exact, the same NaN/inf pattern, |dRGB| <= 1e-5, samples
    exact); Scene.cast and material_data on the KATs, bit for bit; the shadow sets through the any-hit cast, and the
    segments from hit points to light sample points (casts_light: the only segments the shadow grid's root masks hold
    for) through "any_masked" and "any";
  * the schedule arms, each on a fresh Scene: JSRT_HYBRID=0 / 1 on every scene, JSRT_SHADOW_NODE=0 / 1 and JSRT_BUCKET=0
    on the two light scenes, JSRT_SHADE_LDS=0 on shz_phong_children, JSRT_FORCE_EXACT_PICK=1 on shz_path_scatter,
    JSRT_PERSIST=0 on the SDF profile scenes -- equal to the golden and, bit for bit, to the default render;
  * batching: every scene at 44 x 36 under max_paths=1280 (at least 3 batches: data-dependent child counts and unlit
    nodes across batch boundaries, pool sizing) against the oracle and, bit for bit, the unbatched render."""
import numpy as np
import pytest

from oracle import pyoracle
from test_gpu_cast_paths import check_any
from test_gpu_sdfzoo import _check_casts, _check_material
from test_oracle_shadezoo import LIGHT_SCENES, RENDERS, SUB, ZOO, compare_render

pytestmark = pytest.mark.gpu
TO_LIGHT = pyoracle.golden_cast_scenes(SUB, "casts_light")
ARMS = [({"JSRT_HYBRID": "0"}, ZOO), ({"JSRT_HYBRID": "1"}, ZOO),
        ({"JSRT_SHADOW_NODE": "0"}, LIGHT_SCENES), ({"JSRT_SHADOW_NODE": "1"}, LIGHT_SCENES), ({"JSRT_BUCKET": "0"}, LIGHT_SCENES),
        ({"JSRT_SHADE_LDS": "0"}, ["shz_phong_children"]), ({"JSRT_FORCE_EXACT_PICK": "1"}, ["shz_path_scatter"]),
        ({"JSRT_PERSIST": "0"}, ["shz_profiles_sdf", "shz_profiles_all"])]
ARM_CASES = [(env, tag) for env, scenes in ARMS for tag in sorted(RENDERS) if RENDERS[tag]["scene"] in scenes]


@pytest.fixture(scope="module")
def jr():
    import jsraytracer_amd as jr
    return jr


def _render(jr, r, size=None, **kw):
    w, h = size or (r["width"], r["height"])
    sc = jr.Scene(pyoracle.golden_scene(r["scene"], SUB), device=0)
    try:
        rgba, colors, st = sc.render(w, h, r["spp"], r["depth"], r["kind"], r["seed"], **kw)
    finally:
        sc.close()
    assert st["samples"] == w * h * r["spp"]
    return rgba, colors, st


_default = {}


def _default_render(jr, tag, size=None):
    """The frame with no knob set, on a fresh Scene (call before any setenv)."""
    key = (tag, size)
    if key not in _default:
        rgba, colors, _ = _render(jr, RENDERS[tag], size)
        rgba.setflags(write=False)
        colors.setflags(write=False)
        _default[key] = (rgba, colors)
    return _default[key]


@pytest.mark.parametrize("tag", sorted(RENDERS))
def test_gpu_shadezoo_render_matches_reference(jr, tag):
    r = RENDERS[tag]
    gcol, grgba = pyoracle.golden_image(tag, r["width"], r["height"], SUB)
    rgba, colors = _default_render(jr, tag)
    compare_render(rgba, colors, grgba, gcol, tag)


@pytest.mark.parametrize("name", ZOO)
def test_gpu_shadezoo_casts_and_material_match_reference(jr, name):
    sc = jr.Scene(pyoracle.golden_scene(name, SUB), device=0)
    try:
        _check_casts(sc, name, SUB)
        m = pyoracle.golden_material(name, SUB)["material"]
        _check_material(sc.material_data(m["rays"]), m, name)
        s = pyoracle.golden_casts(name, SUB)["sets"][2]
        assert s["name"] == "shadow"
        t, obj = sc.cast_path(s["rays"], s["minD"], s["maxD"], s["transp"], path="any")
        check_any(f"{name}/shadow any", s, t, obj)
    finally:
        sc.close()


@pytest.mark.parametrize("name", TO_LIGHT)
def test_gpu_shadezoo_any_masked_to_light(jr, name):
    """Every scene here has a grid (bounded objects and lights, fewer than 64 top-level objects), so the masked path
    is refused on none; the sets hold segments past the primitives that cast no shadow."""
    (s,) = pyoracle.golden_casts(name, SUB, "casts_light")["sets"]
    assert (s["obj"] >= 0).any() and (s["obj"] < 0).any()
    sc = jr.Scene(pyoracle.golden_scene(name, SUB), device=0)
    try:
        for path in ("any_masked", "any"):
            t, obj = sc.cast_path(s["rays"], s["minD"], s["maxD"], s["transp"], path=path)
            check_any(f"{name}/to_light {path}", s, t, obj)
    finally:
        sc.close()


def _arm_id(c):
    return "+".join(f"{k[5:]}={v}" for k, v in c[0].items()) + "-" + c[1]


@pytest.mark.parametrize("case", ARM_CASES, ids=_arm_id)
def test_gpu_shadezoo_schedule_arm(jr, monkeypatch, case):
    env, tag = case
    r = RENDERS[tag]
    gcol, grgba = pyoracle.golden_image(tag, r["width"], r["height"], SUB)
    rgba0, col0 = _default_render(jr, tag)
    compare_render(rgba0, col0, grgba, gcol, f"{tag} default")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rgba, colors, _ = _render(jr, r)
    compare_render(rgba, colors, grgba, gcol, _arm_id(case))
    assert np.array_equal(rgba, rgba0)
    assert np.array_equal(colors.view(np.uint32), col0.view(np.uint32))


@pytest.mark.parametrize("name", ZOO)
def test_gpu_shadezoo_batched_frame(jr, name):
    """44 x 36 (1,920 patch pixels) of the scene's multisampling render under max_paths=1280."""
    tag = next(t for t in sorted(RENDERS) if RENDERS[t]["scene"] == name and RENDERS[t]["kind"] == 1)
    r, size = RENDERS[tag], (44, 36)
    ocol, orgba, _ = pyoracle.render(pyoracle.golden_scene(name, SUB), *size, r["spp"], r["depth"], r["kind"], r["seed"])
    rgba0, col0 = _default_render(jr, tag, size)
    compare_render(rgba0, col0, orgba, ocol, f"{name} 44x36 unbatched")
    rgba, colors, st = _render(jr, r, size, max_paths=1280)
    print(f"{name}: batches {st['batches']} attempts {st['attempts']}")
    assert st["batches"] >= 3
    compare_render(rgba, colors, orgba, ocol, f"{name} 44x36 batched")
    assert np.array_equal(rgba, rgba0)
    assert np.array_equal(colors.view(np.uint32), col0.view(np.uint32))
