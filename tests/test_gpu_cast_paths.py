"""The casts the render's shadow and SDF kernels run, reached one cast at a time (jsrt_cast_path): the any-hit
world_cast ("any"), the same under the wave's shadow-root mask ("any_masked"), the node-per-lane shadow cast
world_any_node ("any_node"), and the SDF scenes' persistent marches ("persistent", "persistent_any") -- against
known answers computed by the reference itself (tests/golden/casts_edge/, casts_light/, casts/).  A closest path gives the reference's distance bit for bit and
its Primitive; an any-hit path is hit exactly where the reference's shadow-casters cast hits, at an accepted
distance inside (minD, maxD)."""
import numpy as np
import pytest

from oracle import pyoracle

EDGE = pyoracle.golden_cast_scenes(kind="casts_edge")
ALL = pyoracle.golden_cast_scenes()
FLAT = ["BoxBall", "cornell_box", "refraction", "spheres050"]   # every root a Primitive, no SDF
SDF = ["SDF_BoxBall", "SDF_Menger"]
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def jr():
    import jsraytracer_amd as jr
    return jr


def check_any(tag, s, t, obj, with_t=True):
    hit = obj != -1
    want = s["obj"] >= 0
    bad = np.flatnonzero(hit != want)
    assert bad.size == 0, f"{tag}: {bad.size} of {len(hit)} any-hit answers differ, first ray {bad[0]}: reference t {s['t'][bad[0]]!r}"
    if with_t:
        lo, hi = np.broadcast_to(s["minD"], len(t)), np.broadcast_to(s["maxD"], len(t))
        assert ((t[hit] > lo[hit]) & (t[hit] < hi[hit])).all(), f"{tag}: an accepted distance outside (minD, maxD)"
        assert np.isinf(t[~hit]).all(), tag


def path_fn(scene, path):
    return lambda rays, a, b, tr: scene.cast_path(rays, a, b, tr, path=path)


@pytest.mark.parametrize("name", EDGE)
def test_any_hit_edge_sets(jr, name):
    kat = pyoracle.golden_casts(name, kind="casts_edge")
    scene = jr.Scene(pyoracle.golden_scene(name), device=0)
    try:
        for s in kat["sets"]:
            if not s["transp"]:
                t, obj = pyoracle.cast_set(path_fn(scene, "any"), s)
                check_any(f"{name}/{s['name']} any", s, t, obj)
    finally:
        scene.close()


@pytest.mark.parametrize("name", ALL)
def test_any_hit_shadow_sets(jr, name):
    """The generic shadow segments of every golden scene through every any-hit path its profile has."""
    s = next(x for x in pyoracle.golden_casts(name)["sets"] if x["name"] == "shadow")
    scene = jr.Scene(pyoracle.golden_scene(name), device=0)
    try:
        ran = []
        for path in ("any", "persistent_any"):
            try:
                t, obj = scene.cast_path(s["rays"], s["minD"], s["maxD"], s["transp"], path=path)
            except jr.JsrtError as e:
                assert "no such cast path" in str(e)
                continue
            check_any(f"{name}/shadow {path}", s, t, obj)
            ran.append(path)
        assert "any" in ran and (("persistent_any" in ran) == name.startswith("SDF_"))
    finally:
        scene.close()


@pytest.mark.parametrize("name", EDGE)
def test_any_masked_to_light(jr, name):
    """Segments from reference hit points to the lights' sample points -- what the shadow-root masks of the shadow
    grid (scene_load.cpp shadow_grid) hold for -- under the wave's mask (wave_root_mask): every 64 consecutive rays
    share an origin, so every wave, the ragged last one included, takes its cell's mask.  A root missing from a
    cell's mask turns a shadowed segment into a lit one.  Every edge scene has a grid (bounded objects and lights,
    at most 64 top-level objects), so the path is refused on none.  The unmasked cast runs on the same segments."""
    (s,) = pyoracle.golden_casts(name, kind="casts_light")["sets"]
    scene = jr.Scene(pyoracle.golden_scene(name), device=0)
    try:
        for path in ("any_masked", "any"):
            t, obj = scene.cast_path(s["rays"], s["minD"], s["maxD"], s["transp"], path=path)
            check_any(f"{name}/to_light {path}", s, t, obj)
    finally:
        scene.close()


@pytest.mark.parametrize("name", FLAT)
def test_any_node_from_hit(jr, name):
    """Groups of 4 shadow rays sharing a reference hit point, one group per lane (world_any_node<PF, 4>): the
    from_hit groups over the shadow range and, shadow casters only, over from_hit's and from_hit.eps's own ranges
    (minD 0 and 0.0001, no far limit; expected from the oracle, which the CPU suite pins to the reference on these
    rays), and the light segments of casts_light/ in fours, as k_shadow_node casts them."""
    blob = pyoracle.golden_scene(name)
    by = {x["name"]: x for x in pyoracle.golden_casts(name, kind="casts_edge")["sets"]}
    (light,) = pyoracle.golden_casts(name, kind="casts_light")["sets"]
    m = len(light["rays"]) // 4 * 4
    sets = [("from_hit.shadow", by["from_hit.shadow"]),
            ("to_light", {**light, "rays": light["rays"][:m], "t": light["t"][:m], "obj": light["obj"][:m]})]
    for k in ("from_hit", "from_hit.eps"):
        t, obj = pyoracle.cast(blob, by[k]["rays"], by[k]["minD"], by[k]["maxD"], False)
        sets.append((k + " (shadow casters)", {**by[k], "t": t, "obj": obj}))
    scene = jr.Scene(blob, device=0)
    try:
        for tag, s in sets:
            assert 0 < int((s["obj"] >= 0).sum()) < len(s["obj"]), tag
            t, obj = scene.cast_path(s["rays"], s["minD"], s["maxD"], False, path="any_node")
            check_any(f"{name}/{tag} any_node", s, t, obj, with_t=False)
    finally:
        scene.close()


@pytest.mark.parametrize("name", ["bunny", "Aggregates", "SDF_BoxBall"])
def test_any_node_refused_off_flat_scenes(jr, name):
    kat = pyoracle.golden_casts(name, kind="casts_edge")
    s = next(x for x in kat["sets"] if x["name"] == "from_hit.shadow")
    scene = jr.Scene(pyoracle.golden_scene(name), device=0)
    try:
        with pytest.raises(jr.JsrtError, match="no such cast path"):
            scene.cast_path(s["rays"], s["minD"], s["maxD"], False, path="any_node")
    finally:
        scene.close()


@pytest.mark.parametrize("name", SDF)
def test_persistent_edge_sets(jr, name):
    kat = pyoracle.golden_casts(name, kind="casts_edge")
    scene = jr.Scene(pyoracle.golden_scene(name), device=0)
    try:
        for s in kat["sets"]:
            tag = f"{name}/{s['name']}"
            t, obj = pyoracle.cast_set(path_fn(scene, "persistent"), s)
            bad = np.flatnonzero((t.view(np.uint64) != s["t"].view(np.uint64)) | (obj != s["obj"]))
            assert bad.size == 0, (f"{tag} persistent: {bad.size} of {len(t)} casts differ, first ray {bad[0]}: "
                                   f"t {t[bad[0]]!r} vs {s['t'][bad[0]]!r}, obj {obj[bad[0]]} vs {s['obj'][bad[0]]}")
            if not s["transp"]:
                t, obj = pyoracle.cast_set(path_fn(scene, "persistent_any"), s)
                check_any(f"{tag} persistent_any", s, t, obj)
        # fewer rays than one wave: the refill runs dry at once
        s = next(x for x in kat["sets"] if x["name"] == "box_features")
        t, obj = scene.cast_path(s["rays"][:37], s["minD"], s["maxD"], True, path="persistent")
        assert (t.view(np.uint64) == s["t"][:37].view(np.uint64)).all() and (obj == s["obj"][:37]).all()
        s = next(x for x in kat["sets"] if x["name"] == "box_features.shadow")
        t, obj = scene.cast_path(s["rays"][:37], s["minD"], s["maxD"], False, path="persistent_any")
        check_any(f"{name}/box_features.shadow[:37] persistent_any", {**s, "obj": s["obj"][:37], "t": s["t"][:37]}, t, obj)
    finally:
        scene.close()
