"""The HIP path on the SDF zoo (tests/golden/sdfzoo; tests/test_oracle_sdfzoo.py describes the scenes): trees that
match no recognised program form, so the device's program VM (device_common.h sdf_run's interpreter loop) does the
work -- against the reference's own known answers, not against the oracle:
  * World.cast (t as u64 bits, obj), material_data (normal, position, uv[:2], bary, basecolor bit for bit on hits),
    SDF.distance bit for bit, and the 28 x 20 renders (RGBA8 exact, the same NaN/inf pattern, |dRGB| <= 1e-5);
  * the loader's report on the live Scene: zoo roots are form 0;
  * the load-time A/B knobs JSRT_SDF_NOFORMS=1, JSRT_SDF_NOFUSE=1, JSRT_SDF_CROSS=0, JSRT_SDF_N4=0, each on a fresh
    Scene of every zoo scene and of the reference's seven SDF scenes: SDF.distance, casts and material_data still
    the reference's, bit for bit; SDF_Menger also on 4,096 rays from inside the sponge against the oracle;
  * the schedule arms on zoo_mixed (one form root, VM roots, an SDF primitive inside an Aggregate: waves hold several
    programs): JSRT_HYBRID=1, JSRT_PERSIST=0 and both equal the golden and, bit for bit, the default render;
  * a ninth nested smooth combinator is refused at Scene()."""
import numpy as np
import pytest

from oracle import pyoracle
from test_oracle_sdfzoo import REFERENCE_SDF, RENDERS, SUB, ZOO, ZOO_FORMS, _diff_rows, compare_render, ninth_smooth_level

pytestmark = pytest.mark.gpu
KNOBS = [("JSRT_SDF_NOFORMS", "1"), ("JSRT_SDF_NOFUSE", "1"), ("JSRT_SDF_CROSS", "0"), ("JSRT_SDF_N4", "0")]
SCENES = [(n, SUB) for n in ZOO] + [(n, None) for n in REFERENCE_SDF]
MIXED = "zoo_mixed_incremental_28x20_s2_d4_seed1"


@pytest.fixture(scope="module")
def jr():
    import jsraytracer_amd as jr
    return jr


def _check_casts(sc, name, sub):
    for s in pyoracle.golden_casts(name, sub)["sets"]:
        t, obj = sc.cast(s["rays"], s["minD"], s["maxD"], s["transp"])
        bad = np.flatnonzero((obj != s["obj"]) | (t.view(np.uint64) != s["t"].view(np.uint64)))
        assert bad.size == 0, (f"{name}.{s['name']}: {bad.size} of {len(t)} differ, first ray {bad[0]} {s['rays'][bad[0]]}: "
                               f"{t[bad[0]]!r} obj {obj[bad[0]]} vs {s['t'][bad[0]]!r} obj {s['obj'][bad[0]]}")


def _check_material(got, m, name):
    assert np.array_equal(got["obj"], m["obj"])
    assert np.array_equal(got["t"].view(np.uint64), m["t"].view(np.uint64))
    hit = m["obj"] >= 0
    for f, cols in (("normal", 4), ("position", 4), ("uv", 2), ("bary", 3), ("basecolor", 3)):
        bad = _diff_rows(got[f][hit, :cols], m[f][hit, :cols])
        assert bad.size == 0, (f"{name}.{f}: {bad.size} of {int(hit.sum())} hits differ, first: ray {m['rays'][hit][bad[0]]} "
                               f"{got[f][hit][bad[0]]} vs {m[f][hit][bad[0]]}")
    assert np.isnan(got["normal"][~hit]).all()


def _check_distances(sc, kat, name):
    assert kat["sdf"]
    for e in kat["sdf"]:
        d = sc.sdf_distance(e["obj"], e["points"])
        bad = np.flatnonzero(d.view(np.uint64) != e["distance"].view(np.uint64))
        assert bad.size == 0, (f"{name} obj {e['obj']}: {bad.size} of {len(d)} differ, first at {e['points'][bad[0]]}: "
                               f"{d[bad[0]]!r} vs {e['distance'][bad[0]]!r}")


@pytest.mark.parametrize("name", ZOO)
def test_gpu_zoo_matches_reference(jr, name):
    sc = jr.Scene(pyoracle.golden_scene(name, SUB), device=0)
    try:
        assert sc.sdf_forms() == {"all_forms": 0, "roots": ZOO_FORMS[name]}
        kat = pyoracle.golden_material(name, SUB)
        _check_distances(sc, kat, name)
        _check_casts(sc, name, SUB)
        _check_material(sc.material_data(kat["material"]["rays"]), kat["material"], name)
    finally:
        sc.close()


@pytest.mark.parametrize("tag", sorted(RENDERS))
def test_gpu_zoo_render_matches_reference(jr, tag):
    r = RENDERS[tag]
    gcol, grgba = pyoracle.golden_image(tag, r["width"], r["height"], SUB)
    sc = jr.Scene(pyoracle.golden_scene(r["scene"], SUB), device=0)
    try:
        rgba, colors, st = sc.render(r["width"], r["height"], r["spp"], r["depth"], r["kind"], r["seed"])
    finally:
        sc.close()
    compare_render(rgba, colors, grgba, gcol, tag)
    assert st["samples"] == r["width"] * r["height"] * r["spp"]


_dense = {}


def _menger_dense():
    """4,096 rays from inside and around SDF_Menger's sponge (tests/test_gpu_material.py's dense rays) and the
    oracle's material_data of them, computed once."""
    if not _dense:
        rng = np.random.default_rng(29)
        o = (np.array([-3.5, 0.5, -3.5]) + rng.uniform(-1.4, 1.4, (4096, 3))).astype(np.float32)
        d = rng.normal(size=(4096, 3))
        d[:1024] = np.round(d[:1024] * 2) / 2 + 1e-3
        d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
        rays = np.concatenate([o, d], 1)
        want = pyoracle.material_data(pyoracle.golden_scene("SDF_Menger"), rays)
        for a in (rays, *want.values()):
            a.setflags(write=False)
        _dense.update(rays=rays, want=want)
    return _dense["rays"], _dense["want"]


@pytest.mark.parametrize("knob", KNOBS, ids=lambda k: f"{k[0][5:]}={k[1]}")
@pytest.mark.parametrize("scene", SCENES, ids=lambda s: s[0])
def test_gpu_load_knob_keeps_the_answers(jr, monkeypatch, scene, knob):
    name, sub = scene
    kat = pyoracle.golden_material(name, sub)
    if name == "SDF_Menger":
        rays, want = _menger_dense()
    monkeypatch.setenv(*knob)  # read at scene load
    sc = jr.Scene(pyoracle.golden_scene(name, sub), device=0)
    try:
        f = sc.sdf_forms()
        if knob[0] in ("JSRT_SDF_NOFORMS", "JSRT_SDF_NOFUSE"):  # forms are matched on fused programs only
            assert f["all_forms"] == 0 and set(f["roots"].values()) == {0}, f
        elif sub is None:
            assert f["all_forms"] == 1, f
        _check_distances(sc, kat, name)
        _check_casts(sc, name, sub)
        _check_material(sc.material_data(kat["material"]["rays"]), kat["material"], name)
        if name == "SDF_Menger":
            got = sc.material_data(rays)
            assert np.array_equal(got["obj"], want["obj"])
            hit = want["obj"] == 1
            assert hit.sum() > 1250
            for fld, cols in (("normal", 4), ("position", 4), ("basecolor", 3)):
                bad = _diff_rows(got[fld][hit, :cols], want[fld][hit, :cols])
                assert bad.size == 0, f"{fld}: {bad.size} of {int(hit.sum())} differ, first ray {rays[hit][bad[0]]}"
    finally:
        sc.close()


_default = {}


def _default_mixed(jr):
    """zoo_mixed's frame with no knob set, on a fresh Scene (call before any setenv)."""
    if not _default:
        r = RENDERS[MIXED]
        sc = jr.Scene(pyoracle.golden_scene(r["scene"], SUB), device=0)
        try:
            rgba, colors, _ = sc.render(r["width"], r["height"], r["spp"], r["depth"], r["kind"], r["seed"])
        finally:
            sc.close()
        rgba.setflags(write=False)
        colors.setflags(write=False)
        _default.update(rgba=rgba, colors=colors)
    return _default["rgba"], _default["colors"]


@pytest.mark.parametrize("env", [{"JSRT_HYBRID": "1"}, {"JSRT_PERSIST": "0"}, {"JSRT_HYBRID": "1", "JSRT_PERSIST": "0"}],
                         ids=lambda e: "+".join(f"{k[5:]}={v}" for k, v in e.items()))
def test_gpu_schedule_arm_on_mixed_programs(jr, monkeypatch, env):
    r = RENDERS[MIXED]
    gcol, grgba = pyoracle.golden_image(MIXED, r["width"], r["height"], SUB)
    rgba0, col0 = _default_mixed(jr)
    compare_render(rgba0, col0, grgba, gcol, "zoo_mixed default")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc = jr.Scene(pyoracle.golden_scene(r["scene"], SUB), device=0)
    try:
        rgba, colors, st = sc.render(r["width"], r["height"], r["spp"], r["depth"], r["kind"], r["seed"])
    finally:
        sc.close()
    compare_render(rgba, colors, grgba, gcol, f"zoo_mixed {env}")
    assert st["samples"] == r["width"] * r["height"] * r["spp"]
    assert np.array_equal(rgba, rgba0)
    assert np.array_equal(colors.view(np.uint32), col0.view(np.uint32))


def test_gpu_ninth_nested_smooth_combinator_is_refused(jr):
    blob, _ = jr.blob_from_json(ninth_smooth_level())
    with pytest.raises(jr.JsrtError, match="nested 9 deep: the GPU blend stack holds 8"):
        jr.Scene(blob, device=0)
