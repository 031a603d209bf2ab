"""The oracle's World.cast at geometric edges, against known answers computed by the reference itself
(oracle/refharness/make_edge_cast_kats.js -> tests/golden/casts_edge/): rays from and to reference hit
points, ranges that end on the hit distance, zero and near-1e-7 direction components, rays at box corners /
edges / faces and at triangle vertices / edges, tiny, huge and far-away rays.  Distance bit-exact, hit
Primitive exact.  Reference: world.js:7-15, geometry.js:189-209, 368-375, aggregates.js:207-225."""
import gzip
import hashlib
import os

import numpy as np
import pytest

from oracle import pyoracle

EDGE_SCENES = ["AHollowTetrahedron", "AMultipleBVH", "Aggregates", "BoxBall", "SDF_BoxBall", "SDF_Menger", "bunny",
               "cornell_box", "refraction", "spheres050"]
BVH_SCENES = {"AHollowTetrahedron", "AMultipleBVH", "bunny"}
KINDS = {"from_hit", "to_hit", "lim_tie", "axis", "box_features", "scaled"}


def test_edge_scenes_present():
    assert pyoracle.golden_cast_scenes(kind="casts_edge") == EDGE_SCENES


def test_edge_fixtures_no_larger_than_the_generic_ones():
    size = lambda kind: max(os.path.getsize(os.path.join(pyoracle.GOLDEN, kind, f))
                            for f in os.listdir(os.path.join(pyoracle.GOLDEN, kind)))
    assert size("casts_edge") <= size("casts")


@pytest.mark.parametrize("name", EDGE_SCENES)
def test_edge_fixture_conditions(name):
    kat = pyoracle.golden_casts(name, kind="casts_edge")
    kinds = {s["kind"] for s in kat["sets"]}
    assert kinds == KINDS | ({"tri_features"} if name in BVH_SCENES else set())
    for s in kat["sets"]:
        n, tag = s["n"], f"{name}/{s['name']}"
        assert len(s["rays"]) == len(s["t"]) == len(s["obj"]) == n, tag
        assert np.isfinite(s["rays"]).all() and np.any(s["rays"][:, 3:] != 0, axis=1).all(), tag
        assert not np.isnan(s["t"]).any(), tag
        assert s["dropped"] <= 0.01 * (n + s["dropped"]), tag
        hits = int((s["obj"] >= 0).sum())
        if s["transp"]:
            assert hits >= 50 and n - hits >= 50, f"{tag}: {hits} hits of {n}"
        else:       # the any-hit tests rest on these: a set of misses only would check nothing
            assert 0 < hits < n, f"{tag}: {hits} hits of {n}"
        if s["kind"] == "lim_tie":
            assert 0 < hits < n, tag
            assert np.ndim(s["minD"]) == 1 and np.ndim(s["maxD"]) == 1, tag
        elif not s["transp"]:
            assert (s["minD"], s["maxD"]) == (0.0001, 1.0), tag
        if s["name"] == "tri_features":
            other = int(((s["obj"] >= 0) & (s["aim"] >= 0) & (s["obj"] != s["aim"])).sum())
            assert other >= 20, f"{tag}: {other} rays hit another triangle than the one aimed at"
        if s["kind"] == "from_hit":      # groups of 4 consecutive rays share an origin
            o = s["rays"][:, :3].reshape(-1, 4, 3)
            assert n % 4 == 0 and (o == o[:, :1]).all(), tag
    # the shadow twin of every kind is there, on the same rays
    by = {s["name"]: s for s in kat["sets"]}
    for k in kinds:
        assert by[k + ".shadow"]["transp"] is False and by[k]["transp"] is True
        if k != "lim_tie":
            assert by[k + ".shadow"]["rays"] is by[k]["rays"]


@pytest.mark.parametrize("name", EDGE_SCENES)
def test_oracle_edge_cast_matches_reference(name):
    kat = pyoracle.golden_casts(name, kind="casts_edge")
    blob = pyoracle.golden_scene(name)
    assert hashlib.sha256(blob).hexdigest() == kat["blob_sha256"], "KATs were made from another export of the scene"
    for s in kat["sets"]:
        t, obj = pyoracle.cast_set(lambda rays, a, b, tr: pyoracle.cast(blob, rays, a, b, tr), s)
        bad = np.flatnonzero((t.view(np.uint64) != s["t"].view(np.uint64)) | (obj != s["obj"]))
        assert bad.size == 0, (f"{name}/{s['name']}: {bad.size} of {len(t)} casts differ, first ray {bad[0]}: "
                               f"t {t[bad[0]]!r} vs {s['t'][bad[0]]!r}, obj {obj[bad[0]]} vs {s['obj'][bad[0]]}")


# ---- tests/golden/casts_light/ (make_light_cast_kats.js): segments from reference hit points to light samples

def test_light_scenes_present():
    assert pyoracle.golden_cast_scenes(kind="casts_light") == EDGE_SCENES


@pytest.mark.parametrize("name", EDGE_SCENES)
def test_light_fixture_conditions_and_oracle(name):
    kat = pyoracle.golden_casts(name, kind="casts_light")
    blob = pyoracle.golden_scene(name)
    assert hashlib.sha256(blob).hexdigest() == kat["blob_sha256"], "KATs were made from another export of the scene"
    assert os.path.getsize(os.path.join(pyoracle.GOLDEN, "casts_light", name + ".json.gz")) <= max(
        os.path.getsize(os.path.join(pyoracle.GOLDEN, "casts", f)) for f in os.listdir(os.path.join(pyoracle.GOLDEN, "casts")))
    (s,) = kat["sets"]
    n, g = s["n"], s["group"]
    assert s["name"] == "to_light" and (s["minD"], s["maxD"], s["transp"]) == (0.0001, 1.0, False)
    assert len(s["rays"]) == len(s["t"]) == len(s["obj"]) == n and s["dropped"] == 0
    assert np.isfinite(s["rays"]).all() and np.any(s["rays"][:, 3:] != 0, axis=1).all() and not np.isnan(s["t"]).any()
    assert g == 64 and 0 < n % g < g and n <= 4000, "waves of 64 rays, a ragged last one, a few thousand rays"
    o = s["rays"][:, :3]
    assert (o == o[np.arange(n) // g * g]).all(), "the rays of a group of 64 share their origin"
    hits = int((s["obj"] >= 0).sum())
    assert hits >= 50 and n - hits >= 50, f"{name}/to_light: {hits} shadowed segments of {n}"
    t, obj = pyoracle.cast(blob, s["rays"], s["minD"], s["maxD"], s["transp"])
    bad = np.flatnonzero((t.view(np.uint64) != s["t"].view(np.uint64)) | (obj != s["obj"]))
    assert bad.size == 0, (f"{name}/to_light: {bad.size} of {n} casts differ, first ray {bad[0]}: "
                           f"t {t[bad[0]]!r} vs {s['t'][bad[0]]!r}, obj {obj[bad[0]]} vs {s['obj'][bad[0]]}")
