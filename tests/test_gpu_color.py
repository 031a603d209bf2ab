"""World.color of caller-supplied rays on the GPU (include/jsrt_color.h): Scene.color and
Scene.camera_rays.
  1. the reference's own World.color per ray (tests/golden/colors/, tools/make_color_kats.js): every schedule and
     cast path, depth 1 and the scene's maxRecursionDepth, two samples per ray;
  2. the loop closed with the renderer and the pinned oracle: color(camera_rays(sample=s), keys=pixels, sample0=s),
     accumulated on the host in the renderer's order, is the frame jsrt_render and the oracle produce, bit for bit;
  3. a ray's colour depends on (ray, key, sample) alone: not on its place in the batch or on the batch's size;
  4. max_paths batching (three batches and a ragged last one) and the sample0 / spp split change no bit;
  5. edges: depth 0, misses, n = 0, device tensors in and out;
  6. a color call leaves the scene's renders as they were."""
import base64
import gzip
import json
import os

import numpy as np
import pytest

from oracle import pyoracle

pytestmark = pytest.mark.gpu
COLORS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "colors")
KAT_SCENES = ["cornell_box_path", "refraction", "Aggregates", "AMultipleBVH", "SDF_Combinations", "SDF_Menger",
              "BoxBall_DOF", "BoxBall_path", "shz_solid_transparent"]
W, H = 24, 16


@pytest.fixture(scope="module")
def jr():
    import jsraytracer_amd as jr
    return jr


def _blob(name):
    return pyoracle.golden_scene(name, sub="shadezoo" if name.startswith("shz_") else None)


_scenes = {}


def _scene(jr, name):
    if name not in _scenes:
        _scenes[name] = jr.Scene(_blob(name), device=0)
    return _scenes[name]


def _kat(name):
    with gzip.open(os.path.join(COLORS, name + ".json.gz"), "rt") as f:
        k = json.load(f)
    n, ns, nd = k["n"], k["samples"], len(k["depths"])
    k["rays"] = np.frombuffer(base64.b64decode(k["rays"]), np.float32).reshape(n, 6)
    k["hit"] = np.frombuffer(base64.b64decode(k["hit"]), np.uint8).astype(bool)
    k["rgb"] = np.frombuffer(base64.b64decode(k["rgb"]), np.float32).reshape(nd, n, ns, 3)
    return k


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def test_color_kat_files_are_the_committed_scenes():
    assert sorted(f[:-8] for f in os.listdir(COLORS)) == sorted(KAT_SCENES)


@pytest.mark.parametrize("name", KAT_SCENES)
def test_color_matches_reference(jr, name):
    """README's bar for float colour: within 1e-5 absolute (in practice bit-exact; the count of values that are not
    bit-identical is printed)."""
    import hashlib
    k = _kat(name)
    blob = _blob(name)
    assert hashlib.sha256(blob).hexdigest() == k["blob_sha256"]
    hit, n = k["hit"], k["n"]
    assert k["samples"] == 2 and 2 * int(hit.sum()) >= n
    sc = _scene(jr, name)
    for d, depth in enumerate(k["depths"]):
        want = k["rgb"][d]
        # the fixture's own properties (asserted by its generator too): a constant or key-blind output cannot pass
        assert np.isfinite(want).all()
        rows = want[hit].reshape(int(hit.sum()), -1)
        _, inv, cnt = np.unique(_bits(rows), axis=0, return_inverse=True, return_counts=True)
        assert 4 * int((cnt[inv.reshape(-1)] == 1).sum()) >= int(hit.sum())
        if name == "cornell_box_path":
            assert 4 * int((_bits(want[hit, 0]) != _bits(want[hit, 1])).any(-1).sum()) >= int(hit.sum())
        got = sc.color(k["rays"], max_depth=depth, seed=k["seed"], spp=2)
        assert got.shape == (n, 2, 3) and got.dtype == np.float32
        notbit = int((_bits(got) != _bits(want)).sum())
        err = float(np.abs(got.astype(np.float64) - want).max())
        print(f"{name} depth {depth}: {notbit} of {want.size} values not bit-identical, max |d| = {err:.3g}")
        assert np.isfinite(got).all()
        assert err <= 1e-5, f"{name} depth {depth}: max |d| = {err}, {notbit} values differ"
        # a miss is World.bg_color: one colour for every missing ray, whatever its key and sample
        if (~hit).any():
            assert (_bits(got[~hit]) == _bits(got[~hit][0, 0])).all()


def _accumulate(kind, samples):
    """The renderer's f32 accumulation of a pixel's samples in order and its final colour (renderers.js:52-61 Random,
    :93-98 Incremental; render_levels.h accumulate, render.hip k_final)."""
    spp = len(samples)
    acc = np.zeros_like(samples[0])
    for c in samples:
        if kind == 2:
            acc = acc + (c.astype(np.float64) * (1.0 / spp)).astype(np.float32)
        else:
            c0 = c.copy()
            yz = c0[:, 1:]
            yz[np.isnan(yz) | (yz == 0)] = 0.0  # to4(true): `x || 0`
            acc = acc + c0
    return (acc.astype(np.float64) * (1.0 / spp)).astype(np.float32) if kind == 1 else acc


@pytest.mark.parametrize("name,kind,spp", [("refraction", 0, 1), ("cornell_box_path", 1, 2), ("BoxBall_DOF", 2, 2),
                                            ("BoxBall_path", 1, 2)])
def test_color_of_camera_rays_is_the_render(jr, name, kind, spp):
    blob = _blob(name)
    sc = _scene(jr, name)
    depth = sc.header()["max_depth"]
    keys = np.arange(W * H, dtype=np.uint32)
    samples = []
    for s in range(spp):
        rays = sc.camera_rays(W, H, kind=kind, seed=3, sample=s)
        assert rays.shape == (W * H, 6) and np.isfinite(rays).all()
        samples.append(sc.color(rays, keys, max_depth=depth, seed=3, sample0=s)[:, 0])
    if spp > 1:  # the jitter (and the DOF draws) are keyed by the sample
        assert not _same(sc.camera_rays(W, H, kind=kind, seed=3, sample=0), sc.camera_rays(W, H, kind=kind, seed=3, sample=1))
    mine = samples[0] if kind == 0 else _accumulate(kind, samples)
    _, colors, _ = sc.render(W, H, spp, depth, kind, 3)
    ocol, _, _ = pyoracle.render(blob, W, H, spp, depth, kind, 3)
    assert _same(mine, colors[..., :3].reshape(-1, 3)), "differs from jsrt_render's colors_f32"
    assert _same(mine, ocol[..., :3].reshape(-1, 3)), "differs from the oracle's colours"


# flat (hybrid chain), path tracing (hybrid chain; BoxBall_path: the plain chain, no material has two children), SDF (tree)
INDEX_SCENES = ["refraction", "cornell_box_path", "BoxBall_path", "SDF_Combinations"]
_base = {}


def _base_colors(jr, name):
    """The scene's 24 x 16 camera rays, keyed by pixel, two samples each: computed once per scene."""
    if name not in _base:
        sc = _scene(jr, name)
        rays = sc.camera_rays(W, H, kind=1, seed=5, sample=0)
        _base[name] = (rays, sc.color(rays, np.arange(W * H, dtype=np.uint32), seed=5, spp=2))
    return _base[name]


@pytest.mark.parametrize("name", INDEX_SCENES)
@pytest.mark.parametrize("n", [1, 63, 64, 257])
def test_color_depends_on_ray_and_key_only(jr, name, n):
    sc = _scene(jr, name)
    rays, base = _base_colors(jr, name)
    rng = np.random.default_rng(n)
    idx = rng.integers(0, len(rays), n).astype(np.uint32)  # with repeats: the same ray and key at several places
    if n > 1:
        idx[-1] = idx[0]
    got = sc.color(rays[idx], idx, seed=5, spp=2)
    assert _same(got, base[idx])
    p = rng.permutation(n)
    assert _same(sc.color(rays[idx][p], idx[p], seed=5, spp=2), got[p])
    # and the key matters: another key draws other numbers (the path-tracing scene scatters)
    if name == "cornell_box_path" and n >= 63:
        assert not _same(sc.color(rays[idx], idx + 1000, seed=5, spp=2), got)


@pytest.mark.parametrize("name", INDEX_SCENES)
def test_color_batches_change_no_bit(jr, name):
    sc = _scene(jr, name)
    rays, base = _base_colors(jr, name)
    idx = (np.arange(600) % len(rays)).astype(np.uint32)
    one, st = {}, {}
    whole = sc.color(rays[idx], idx, seed=5, spp=2, stats=one)
    split = sc.color(rays[idx], idx, seed=5, spp=2, max_paths=512, stats=st)
    assert one["batches"] == 1 and st["batches"] >= 3 and st["samples"] == 1200
    assert _same(whole, base[idx]) and _same(split, whole)
    assert _same(sc.color(rays[idx], idx, seed=5, sample0=1, spp=1, max_paths=512)[:, 0], whole[:, 1])
    assert _same(sc.color(rays[idx], seed=5, spp=2)[:len(rays)], sc.color(rays, seed=5, spp=2))  # keys None: the index


def test_color_edges(jr):
    import torch
    sc = _scene(jr, "refraction")
    rays, base = _base_colors(jr, "refraction")
    keys = np.arange(len(rays), dtype=np.uint32)
    black = sc.color(rays, keys, max_depth=0, spp=2)
    assert black.shape == (len(rays), 2, 3) and not black.any()
    empty = sc.color(np.zeros((0, 6), np.float32))
    assert empty.shape == (0, 1, 3) and empty.dtype == np.float32
    dev = torch.device("cuda", 0)
    t = sc.color(torch.from_numpy(rays).to(dev), torch.from_numpy(keys.view(np.int32)).to(dev), seed=5, spp=2)
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.shape == (len(rays), 2, 3)
    assert _same(t.cpu().numpy(), base)
    t0 = sc.color(torch.zeros((0, 6), device=dev))
    assert t0.is_cuda and t0.shape == (0, 1, 3)
    with pytest.raises(jr.JsrtError, match="maxRecursionDepth above"):
        sc.color(rays, max_depth=17)
    with pytest.raises(jr.JsrtError, match="one key per ray"):
        sc.color(rays, keys[:-1])
    # jsrt_camera_rays refuses a null output (after the params are resolved, so on a real scene) and a bad size
    import ctypes
    from jsraytracer_amd import _native
    L = _native.color_api()
    assert L.jsrt_camera_rays(sc._h, ctypes.byref(sc.params(8, 8, device=0)), 0, None) == -1
    assert _native.last_error() == "out_rays is NULL"
    bad = np.zeros((1, 6), np.float32)
    assert L.jsrt_camera_rays(sc._h, ctypes.byref(sc.params(8, 8, kind=3, device=0)), 0, bad.ctypes.data) == -1
    assert _native.last_error() == "unknown renderer kind"


@pytest.mark.parametrize("name", INDEX_SCENES)
def test_color_leaves_renders_alone(jr, name):
    sc = _scene(jr, name)
    rays, base = _base_colors(jr, name)
    rgba0, col0, _ = sc.render(W, H, 2, 0, 1, 7)
    assert _same(sc.color(rays, np.arange(len(rays), dtype=np.uint32), seed=5, spp=2), base)
    rgba1, col1, _ = sc.render(W, H, 2, 0, 1, 7)
    assert rgba0.tobytes() == rgba1.tobytes() and col0.tobytes() == col1.tobytes()
