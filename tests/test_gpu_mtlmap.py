"""The MTL texture-map scene on the GPU (tests/golden/mtlmap/, built and rendered by the reference itself): the
reference-exported blob at the parity bar of tests/test_gpu_parity.py under both renderers (RGBA8 identical, the same
non-finite pattern, |dRGB| <= 1e-5), and the natively attached blob rendering bit-identically to it."""
import numpy as np
import pytest

import mtlmap_kats as mk

pytestmark = pytest.mark.gpu
TOL = 1e-5  # tests/test_gpu_parity.py


@pytest.fixture(scope="module")
def jr():
    import jsraytracer_amd as jr
    return jr


def _render(jr, blob, name):
    r = mk.index()["renders"][name]
    return jr.Scene(blob, device=0).render(r["width"], r["height"], r["spp"], r["depth"], r["kind"], r["seed"])


@pytest.mark.parametrize("name", mk.RENDERS)
def test_scene_matches_reference_render(jr, name):
    rgba, colors, _ = _render(jr, mk.blob("full"), name)
    gcol, grgba = mk.golden_image(name)
    bad = (rgba != grgba).any(-1)
    fin = np.isfinite(gcol[..., :3])
    same_fin = np.array_equal(np.isfinite(colors[..., :3]), fin)
    both = fin & np.isfinite(colors[..., :3])
    err = float(np.abs(colors[..., :3][both] - gcol[..., :3][both]).max())
    print(f"mtlmap {name}: {int(bad.sum())} RGBA8 pixels differ, non-finite pattern equal {same_fin}, max |dRGB| {err}")
    assert not bad.any(), f"{name}: {int(bad.sum())} RGBA8 pixels differ"
    assert same_fin, f"{name}: NaN/inf pattern differs"
    assert err <= TOL, f"{name}: max |dRGB| {err}"


@pytest.mark.parametrize("name", mk.RENDERS)
def test_native_attach_renders_like_the_reference_export(jr, name):
    blob, _ = jr.attach_obj(mk.blob("skel"), mk.text("scene.obj"), mtl_texts=[mk.text("scene.mtl")], textures=mk.textures())
    a, b = _render(jr, blob, name), _render(jr, mk.blob("full"), name)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
