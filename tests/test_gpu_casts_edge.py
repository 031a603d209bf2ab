"""World.cast on the GPU at geometric edges (jsrt_cast -> world_cast / bvh_cast / the SDF march, with their
f32 filters and culls), against known answers computed by the reference itself
(oracle/refharness/make_edge_cast_kats.js -> tests/golden/casts_edge/, the sets tests/test_oracle_casts_edge.py
describes).  Distance bit-exact, hit Primitive exact."""
import numpy as np
import pytest

from oracle import pyoracle

SCENES = pyoracle.golden_cast_scenes(kind="casts_edge")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def jr():
    import jsraytracer_amd as jr
    return jr


@pytest.mark.parametrize("name", SCENES)
def test_gpu_edge_cast_matches_reference(jr, name):
    kat = pyoracle.golden_casts(name, kind="casts_edge")
    scene = jr.Scene(pyoracle.golden_scene(name), device=0)
    try:
        for s in kat["sets"]:
            t, obj = pyoracle.cast_set(scene.cast, s)
            bad = np.flatnonzero((t.view(np.uint64) != s["t"].view(np.uint64)) | (obj != s["obj"]))
            assert bad.size == 0, (f"{name}/{s['name']}: {bad.size} of {len(t)} casts differ, first ray {bad[0]}: "
                                   f"t {t[bad[0]]!r} vs {s['t'][bad[0]]!r}, obj {obj[bad[0]]} vs {s['obj'][bad[0]]}")
    finally:
        scene.close()
