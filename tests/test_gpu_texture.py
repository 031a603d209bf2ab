"""Textures on the GPU against the reference's own TextureMaterialColor (tests/golden/texture/, written by
tools/make_texture_fixtures.js from the reference's code; the oracle does not know textures):

  * Scene.material_color (k_material_color: mc_eval with the sampler of texture_sample.h) on every known answer,
    bit for bit, NaN where the reference returns NaN;
  * the four 32 x 24 scenes -- flat (SimpleRenderer, the LDS-staged k_shade), box (Incremental 4 spp, a textured
    diffusivity through the hybrid chain, k_shadow_node and the HAND_DIFF plane), mesh (a BVH of UV-mapped
    triangles, the tree schedule), cylinder (a Checkerboard of two textures) -- at the parity bar of
    tests/test_gpu_parity.py: RGBA8 identical, the same non-finite pattern, |dRGB| <= 1e-5;
  * the box under the schedule knobs, the flat scene in column partitions, the mesh textured by set_texture, and a
    texture in a refused slot.
"""
import numpy as np
import pytest

import texture_kats as tk

pytestmark = pytest.mark.gpu
TOL = 1e-5  # tests/test_gpu_parity.py


@pytest.fixture(scope="module")
def jr():
    import jsraytracer_amd as jr
    return jr


@pytest.fixture(scope="module")
def kat_scene(jr):
    return jr.Scene(tk.blob("kats"), device=0)


def _render(jr, blob, name, **kw):
    r = tk.scene_index()[name]
    return jr.Scene(blob, device=0).render(r["width"], r["height"], r["spp"], r["depth"], r["kind"], r["seed"], **kw)


_default = {}


def _default_render(jr, name):
    if name not in _default:
        _default[name] = _render(jr, tk.blob(name), name)
    return _default[name]


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


@pytest.mark.parametrize("cid", [c["id"] for c in tk.kats()])
def test_material_color_equals_reference(kat_scene, cid):
    c = next(x for x in tk.kats() if x["id"] == cid)
    got = kat_scene.material_color(c["mcolor"], c["uv"])
    bad = tk.same_bits(got, c["want"]).any(1)
    assert not bad.any(), (f"{cid}: {int(bad.sum())} of {len(bad)} differ, first uv {c['uv'][bad][0]} got {got[bad][0]} "
                           f"want {c['want'][bad][0]}")


def test_material_color_of_plain_records(jr, kat_scene):
    """Solid and Scaled(solid) records through the same entry point (the minimal world's PhongMaterial(white, 0.5,
    0.5)); an index out of range is an error."""
    mc = tk.records(tk.blob("kats"), "MCOL", tk.MCOL_DTYPE)
    solid = next(i for i, r in enumerate(mc) if r["kind"] == 1)
    scaled = next(i for i, r in enumerate(mc) if r["kind"] == 2 and mc[r["a"]]["kind"] == 1)
    uv = np.array([[0.25, 0.75], [np.nan, 2.0]], np.float32)
    assert np.array_equal(kat_scene.material_color(solid, uv), np.tile(mc[solid]["vec"][:3], (2, 1)))
    want = (mc[mc[scaled]["a"]]["vec"][:3].astype(np.float64) * mc[scaled]["scalar"]).astype(np.float32)
    assert np.array_equal(kat_scene.material_color(scaled, uv), np.tile(want, (2, 1)))
    with pytest.raises(jr.JsrtError):
        kat_scene.material_color(len(mc), uv)


@pytest.mark.parametrize("name", tk.SCENES)
def test_scene_matches_reference_render(jr, name):
    rgba, colors, _ = _default_render(jr, name)
    gcol, grgba = tk.golden_image(name)
    bad = (rgba != grgba).any(-1)
    assert not bad.any(), f"{name}: {int(bad.sum())} RGBA8 pixels differ, max {int(np.abs(rgba.astype(int) - grgba).max())}"
    fin = np.isfinite(gcol[..., :3])
    assert np.array_equal(np.isfinite(colors[..., :3]), fin), f"{name}: NaN/inf pattern differs"
    err = float(np.abs(colors[..., :3][fin] - gcol[..., :3][fin]).max())
    assert err <= TOL, f"{name}: max |dRGB| {err}"


@pytest.mark.parametrize("knob", ["JSRT_HYBRID=0", "JSRT_HYBRID=1", "JSRT_SHADOW_NODE=0", "JSRT_SHADE_LDS=0"])
def test_box_schedule_knobs_change_nothing(jr, monkeypatch, knob):
    """The textured wall through the tree, the hybrid chain, k_shadow instead of k_shadow_node, and k_shade without
    the LDS-staged tables: bit for bit the default render."""
    ref = _default_render(jr, "box")
    k, v = knob.split("=")
    monkeypatch.setenv(k, v)
    assert _same(_render(jr, tk.blob("box"), "box"), ref)


def test_flat_partitions_composite_to_the_whole(jr):
    full = _default_render(jr, "flat")
    W = tk.scene_index()["flat"]["width"]
    comp, ccol = np.zeros_like(full[0]), np.full_like(full[1], np.nan)
    for k in range(3):
        part, pcol, _ = _render(jr, tk.blob("flat"), "flat", x_offset=k, x_delt=3)
        assert not part[:, [c for c in range(W) if c % 3 != k]].any()
        comp[:, k::3] = part[:, k::3]
        ccol[:, k::3] = pcol[:, k::3]
    assert _same((comp, ccol), full)


def test_mesh_textured_by_set_texture_renders_identically(jr):
    want = tk.blob("mesh")
    mc = next(i for i, r in enumerate(tk.records(want, "MCOL", tk.MCOL_DTYPE)) if r["kind"] == tk.MC_TEXTURE)
    (t, img), = tk.textures(want)
    blob = jr.set_texture(tk.blob("mesh_untextured"), mc, img, mode="bilinear", clampU=bool(t["clamp_u"]),
                          clampV=bool(t["clamp_v"]))
    assert _same(_render(jr, blob, "mesh"), _default_render(jr, "mesh"))
    plain = _render(jr, tk.blob("mesh_untextured"), "mesh")
    assert not np.array_equal(plain[0], _default_render(jr, "mesh")[0]), "the texture shows in the image"


def test_texture_in_a_refused_slot_raises(jr):
    b = bytearray(tk.blob("flat"))
    mc = next(i for i, r in enumerate(tk.records(bytes(b), "MCOL", tk.MCOL_DTYPE)) if r["kind"] == tk.MC_TEXTURE)
    count, off, _ = tk.sections(bytes(b))["MATL"]
    mat = np.frombuffer(b, np.dtype([("kind", "<u4"), ("slots", "<i4", 7), ("rest", "V32")]), count, off)
    mat[0]["slots"][4] = mc  # reflect
    with pytest.raises(jr.JsrtError, match="reflectivity"):
        jr.Scene(bytes(b), device=0)
