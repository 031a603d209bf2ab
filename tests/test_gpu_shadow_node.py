"""k_shadow's two forms -- one lane per light sample (JSRT_SHADOW_NODE=0) and one lane per lit node
(JSRT_SHADOW_NODE=1: k_shadow_node, where the scene allows it: a flat scene with one area light of 2..4 samples;
every other scene keeps the lane-per-sample kernel under either setting) -- against the oracle and against each
other.  Bar (test_gpu_parity): RGBA8 identical, same NaN/inf pattern, |dRGB| <= 1e-5 against the oracle; the two
settings bit for bit equal in rgba and in the f32 colours.

The cases: the hybrid chain with grid-cell buckets, a 4-sample area light, side chains and a HAND_DIFF plane
(cornell_box_path); partly filled last blocks and waves (max_paths=640); fewer lit nodes than one wave (7x5);
the tree schedule with Fresnel kr / refr planes and two point lights (refraction_path, refraction: the
multi-light sums); a Sphere area light (heart: the lane-per-sample form under both settings); a mesh profile
with primitive buckets (bunny); a non-zero ambient term under the node form (cornell_box: Phong walls with
ambient 0.1, the same area light); the unbucketed hand-off (JSRT_BUCKET=0), which reads INFO_LIT from the
node record as before; the one-lane-per-node serial k_shadow (JSRT_SHADOW_SERIAL=1) with the bucketed hand-off,
with a Sphere light and in a BVH profile; and the unstaged analytic k_shade / k_shadow (JSRT_SHADE_LDS=0, read
when the scene is created)."""
import numpy as np
import pytest

from oracle import pyoracle

pytestmark = pytest.mark.gpu
TOL = 1e-5

# (scene, W, H, spp, depth (None: the scene's), seed, render kwargs, environment)
CASES = [
    ("cornell_box_path", 40, 40, 6, 8, 11, {}, {}),
    ("cornell_box_path", 40, 40, 6, 8, 11, {"max_paths": 640}, {}),
    ("cornell_box_path", 7, 5, 3, 8, 11, {}, {}),
    ("refraction_path", 40, 40, 4, None, 3, {}, {}),
    ("heart", 32, 32, 2, None, 5, {}, {}),
    ("bunny", 48, 40, 2, 4, 3, {}, {}),
    ("refraction", 32, 32, 2, None, 4, {}, {}),
    ("cornell_box", 32, 32, 3, None, 6, {}, {}),
    ("cornell_box_path", 40, 40, 6, 8, 11, {}, {"JSRT_BUCKET": "0"}),
    ("cornell_box_path", 40, 40, 6, 8, 11, {}, {"JSRT_SHADOW_SERIAL": "1"}),
    ("heart", 32, 32, 2, None, 5, {}, {"JSRT_SHADOW_SERIAL": "1"}),
    ("bunny", 48, 40, 2, 4, 3, {}, {"JSRT_SHADOW_SERIAL": "1"}),
    ("cornell_box_path", 40, 40, 6, 8, 11, {}, {"JSRT_SHADE_LDS": "0"}),
]


def _id(c):
    extra = "".join(f"_{k}{v}" for k, v in {**c[6], **c[7]}.items())
    return f"{c[0]}_{c[1]}x{c[2]}_s{c[3]}{extra}"


@pytest.fixture(scope="module")
def jr():
    import jsraytracer_amd as jr
    return jr


_oracle = {}


def _reference(name, W, H, spp, depth, seed):
    key = (name, W, H, spp, depth, seed)
    if key not in _oracle:
        ocol, orgba, _ = pyoracle.render(pyoracle.golden_scene(name), W, H, spp, depth, 1, seed)
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
def test_shadow_forms_match_oracle_and_each_other(jr, monkeypatch, case):
    name, W, H, spp, depth, seed, kw, env = case
    blob = pyoracle.golden_scene(name)
    if depth is None:
        depth = pyoracle.scene_header(blob)["max_depth"]
    ocol, orgba = _reference(name, W, H, spp, depth, seed)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got = {}
    for form in ("0", "1"):
        monkeypatch.setenv("JSRT_SHADOW_NODE", form)
        rgba, colors, st = jr.Scene(blob, device=0).render(W, H, spp, depth, 1, seed, **kw)
        _compare(rgba, colors, orgba, ocol, f"{_id(case)} JSRT_SHADOW_NODE={form}")
        assert st["samples"] == W * H * spp
        got[form] = (rgba, colors)
    assert np.array_equal(got["0"][0], got["1"][0])
    assert np.array_equal(got["0"][1].view(np.uint32), got["1"][1].view(np.uint32))
