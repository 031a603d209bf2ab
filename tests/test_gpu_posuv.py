"""PositionalUVMaterial on the GPU against the reference's own class (tests/golden/posuv/, written by
tools/make_posuv_fixtures.js from the reference's code; the oracle does not know the class):

  * Scene.material_uv (k_material_uv: shade_node's surface_data and posuv_map) on every recorded ray of the five
    scenes, bit for bit, has_uv included;
  * the five 32 x 24 scenes -- flat (SimpleRenderer, the LDS-staged k_shade: a Plane, a UnitBox, a Sphere, a nested
    pair, a SolidColor and a Transparent base), flat_plain (flat with a checkerboard for its texture), box
    (Incremental 4 spp, textured PhongPathTracing walls through the hybrid chain, k_shadow_node and the HAND_DIFF
    plane), mesh (a BVH of triangles without `vt` inside a transformed
    Aggregate), sdf (SDF primitives with a basecolor) -- at the parity bar of tests/test_gpu_parity.py: RGBA8
    identical, the same non-finite pattern, |dRGB| <= 1e-5;
  * the box under the schedule knobs, the flat scene in column partitions, and the mesh without its wrapper.
"""
import numpy as np
import pytest

import posuv_kats as pk

pytestmark = pytest.mark.gpu
TOL = 1e-5  # tests/test_gpu_parity.py


@pytest.fixture(scope="module")
def jr():
    import jsraytracer_amd as jr
    return jr


def _render(jr, blob, name, **kw):
    r = pk.scene_index()[name]
    return jr.Scene(blob, device=0).render(r["width"], r["height"], r["spp"], r["depth"], r["kind"], r["seed"], **kw)


_default = {}


def _default_render(jr, name):
    if name not in _default:
        _default[name] = _render(jr, pk.blob(name), name)
    return _default[name]


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


@pytest.mark.parametrize("name", pk.SCENES)
def test_material_uv_equals_reference(jr, name):
    a = pk.uv_answers(name)
    uv, has = jr.Scene(pk.blob(name), device=0).material_uv(a["rays"])
    print(f"{name}: {int(has.sum())} of {len(has)} rays have a UV (reference {int(a['has_uv'].sum())})")
    assert np.array_equal(has, a["has_uv"]), f"{name}: has_uv differs on {int((has != a['has_uv']).sum())} rays"
    bad = pk.same_bits(uv, a["uv"]).any(1)
    print(f"{name}: {int(bad.sum())} of {len(bad)} UV pairs differ")
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {len(bad)} differ, first ray {a['rays'][bad][0]} got {uv[bad][0]} "
                           f"want {a['uv'][bad][0]}")
    assert a["has_uv"].sum() >= 200 and (a["map"] >= 0).sum() >= 80


@pytest.mark.parametrize("name", pk.SCENES)
def test_scene_matches_reference_render(jr, name):
    rgba, colors, _ = _default_render(jr, name)
    gcol, grgba = pk.golden_image(name)
    bad = (rgba != grgba).any(-1)
    fin = np.isfinite(gcol[..., :3])
    same_fin = np.array_equal(np.isfinite(colors[..., :3]), fin)
    both = fin & np.isfinite(colors[..., :3])
    err = float(np.abs(colors[..., :3][both] - gcol[..., :3][both]).max())
    print(f"{name}: {int(bad.sum())} RGBA8 pixels differ, non-finite pattern equal {same_fin}, max |dRGB| {err}")
    assert not bad.any(), f"{name}: {int(bad.sum())} RGBA8 pixels differ, max {int(np.abs(rgba.astype(int) - grgba).max())}"
    assert same_fin, f"{name}: NaN/inf pattern differs"
    assert err <= TOL, f"{name}: max |dRGB| {err}"


@pytest.mark.parametrize("knob", ["JSRT_HYBRID=0", "JSRT_HYBRID=1", "JSRT_SHADOW_NODE=0", "JSRT_SHADE_LDS=0"])
def test_box_schedule_knobs_change_nothing(jr, monkeypatch, knob):
    """The wrapped walls through the tree, the hybrid chain, k_shadow instead of k_shadow_node, and k_shade with the
    mapping table in global memory instead of LDS: bit for bit the default render."""
    ref = _default_render(jr, "box")
    k, v = knob.split("=")
    monkeypatch.setenv(k, v)
    assert _same(_render(jr, pk.blob("box"), "box"), ref)


def test_flat_partitions_composite_to_the_whole(jr):
    full = _default_render(jr, "flat")
    W = pk.scene_index()["flat"]["width"]
    comp, ccol = np.zeros_like(full[0]), np.full_like(full[1], np.nan)
    for k in range(3):
        part, pcol, _ = _render(jr, pk.blob("flat"), "flat", x_offset=k, x_delt=3)
        assert not part[:, [c for c in range(W) if c % 3 != k]].any()
        comp[:, k::3] = part[:, k::3]
        ccol[:, k::3] = pcol[:, k::3]
    assert _same((comp, ccol), full)


def test_mesh_without_its_wrapper_differs(jr):
    """The mesh's triangles pointed at the wrapper's base material (no `vt`: the colour chains then read u = v = 0):
    another image, so the mapping is what the golden shows."""
    b = pk.blob("mesh")
    mat, obj = pk.records(b, "MATL", pk.MATL_DTYPE), pk.records(b, "OBJS", pk.OBJS_DTYPE)
    wrapped = mat["kind"][np.maximum(obj["material"], 0)] == pk.MAT_POSITIONAL_UV
    wrapped &= obj["material"] >= 0
    assert wrapped.sum() == 40
    obj["material"][wrapped] = mat["base"][obj["material"][wrapped]]
    plain = _render(jr, pk.rebuild(b, OBJS=obj), "mesh")
    _, grgba = pk.golden_image("mesh")
    differ = int((plain[0] != grgba).any(-1).sum())
    print(f"mesh without its wrapper: {differ} RGBA8 pixels differ from the golden")
    assert differ > 0
