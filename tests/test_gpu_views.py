"""Many cameras of one scene in one wavefront batch (include/jsrt_views.h): Scene.render_views.

The one rule: view v is, bit for bit, the frame Scene(with_camera(blob, cam_v)).render(...) returns with the same
arguments and the view's seed.
  1. golden: all 5 fixture cameras of tests/golden/views/ (the reference's own frames, tools/make_view_kats.sh) in one
     call, per scene: RGBA8 exact, f32 within TOL (the count of values not bit-identical is printed);
  2. the solo rule against Scene.render of the patched blob, bit for bit, view 0 against the unpatched scene;
  3. a perspective and a depth-of-field camera in one call, on a scene of either kind;
  4. shapes where the generator and the fold can go wrong, against the oracle's render of the patched blob (the
     project's GPU-versus-oracle bar: RGBA8 exact, |dRGB| <= TOL), all three renderer kinds: 7 x 9 frames (63 pixels:
     every wave straddles two views) x 1, 3, 65 views; 1 x 1 x 130 views; 13 x 7 x 3 views at 3 spp with a max_paths
     that ends batches in the middle of a view and cuts the samples into 3 chunks; depth 0 (black); depth 16;
  5. a view's bytes do not depend on nviews, on max_paths or on the schedule knob;
  6. view_seeds: the solo renders at those seeds; none: the call's seed for every view;
  7. the device entry on a non-default stream equals the host result and leaves the scene's renders as they were;
  8. every refused argument returns -1 with a message naming the field."""
import ctypes
import struct

import numpy as np
import pytest

import views_kats as vk
from oracle import pyoracle

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.fixture(scope="module")
def jr():
    import jsraytracer_amd as jr
    return jr


_scenes, _solo, _oracle = {}, {}, {}


def _scene(jr, name):
    if name not in _scenes:
        _scenes[name] = jr.Scene(pyoracle.golden_scene(name), device=0)
    return _scenes[name]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(rgba, col, rgba2, col2):
    return np.array_equal(rgba, rgba2) and np.array_equal(_bits(col), _bits(col2))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _solo_render(jr, name, view, W, H, spp, depth, kind, seed):
    """Scene(with_camera(blob, cam_view)).render(...) on the GPU: (rgba, colors), computed once, read-only."""
    key = (name, view, W, H, spp, depth, kind, seed)
    if key not in _solo:
        if (name, view) not in _scenes:
            _scenes[name, view] = jr.Scene(vk.solo_blob(name, view), device=0)
        rgba, colors, _ = _scenes[name, view].render(W, H, spp, depth, kind, seed)
        _solo[key] = _frozen(rgba, colors)
    return _solo[key]


def _compare(rgba, colors, grgba, gcol, label):
    got, want = colors[..., :3], gcol[..., :3]
    notbit = int(((_bits(got) != _bits(want)) & ~(np.isnan(got) & np.isnan(want))).sum())
    fin = np.isfinite(want)
    err = float(np.abs(got[fin] - want[fin]).max()) if fin.any() and np.isfinite(got[fin]).all() else 0.0
    print(f"{label}: {notbit} of {want.size} f32 values not bit-identical, max |dRGB| = {err:.3g}")
    bad = (rgba != grgba).any(-1)
    assert not bad.any(), f"{label}: {int(bad.sum())} RGBA8 pixels differ"
    assert np.array_equal(np.isfinite(got), fin), f"{label}: NaN/inf pattern differs"
    assert err <= TOL, f"{label}: max |dRGB| {err}"


# ---- 1. the reference's frames ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(vk.SCENES))
def test_views_match_reference(jr, name):
    k = vk.load(name)
    W, H = k["width"], k["height"]
    st = {}
    rgba, colors = _scene(jr, name).render_views(vk.cameras(name), W, H, k["spp"], k["depth"], k["kind"], k["seed"],
                                                 want_colors=True, stats=st)
    assert rgba.shape == (5, H, W, 4) and rgba.dtype == np.uint8 and colors.shape == (5, H, W, 4)
    assert st["samples"] == 5 * W * H * k["spp"] and st["batches"] >= 1 and st["attempts"] >= 1
    assert (colors[..., 3] == 1).all() and (rgba[..., 3] == 255).all()
    for v in range(5):
        grgba, gcol = vk.image(name, v)
        _compare(rgba[v], colors[v], grgba, gcol, f"{name} view {v}")


# ---- 2. the solo rule ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_box_path", "bunny", "BoxBall_DOF"])
def test_view_is_the_solo_render(jr, name):
    k = vk.load(name)
    args = (k["width"], k["height"], k["spp"], k["depth"], k["kind"], k["seed"])
    sc = _scene(jr, name)
    assert sc.camera() == vk.cameras(name)[0] == jr.blob_camera(pyoracle.golden_scene(name))
    rgba, colors = sc.render_views(vk.cameras(name), *args, want_colors=True)
    own_rgba, own_col, _ = sc.render(*args)  # the unpatched scene
    assert _same(rgba[0], colors[0], own_rgba, own_col), f"{name}: view 0 is not the scene's own render"
    for v in range(5):
        assert _same(rgba[v], colors[v], *_solo_render(jr, name, v, *args)), f"{name}: view {v} differs from its solo render"


# ---- 3. mixed camera kinds ----------------------------------------------------------------------------------------
def _oracle_view(name, cam, W, H, spp, depth, kind, seed, key=None):
    """The oracle's (rgba, colors) of the scene with `cam` as its camera; cached under `key` when one is given."""
    if key is None or key not in _oracle:
        import jsraytracer_amd as jr
        col, rgba, _ = pyoracle.render(jr.with_camera(pyoracle.golden_scene(name), cam), W, H, spp, depth, kind, seed)
        if key is None:
            return rgba, col
        _oracle[key] = _frozen(rgba, col)
    return _oracle[key]


@pytest.mark.parametrize("name", ["BoxBall_path", "BoxBall_DOF"])
def test_mixed_camera_kinds(jr, name):
    dof = vk.cameras("BoxBall_DOF")[1]
    own = vk.cameras(name)[0]
    cams = [own.replace(kind=0, focus_distance=0.0, sensor_size=0.0),
            own.replace(kind=1, focus_distance=dof.focus_distance, sensor_size=dof.sensor_size),
            vk.cameras(name)[2].replace(kind=0), vk.cameras(name)[3].replace(kind=1, focus_distance=5.0, sensor_size=0.25)]
    depth = vk.load(name)["depth"]
    rgba, colors = _scene(jr, name).render_views(cams, 20, 12, 2, depth, 1, 7, want_colors=True)
    views = [_oracle_view(name, c, 20, 12, 2, depth, 1, 7) for c in cams]
    for v, (orgba, ocol) in enumerate(views):
        _compare(rgba[v], colors[v], orgba, ocol, f"{name} mixed view {v} (kind {cams[v].kind})")
    assert (views[0][0] != views[1][0]).any()  # depth of field changes the image: the kind is read per view


# ---- 4. shapes ----------------------------------------------------------------------------------------------------
def _many_cameras(name, n):
    """n distinct cameras around the scene's own: the fixture's 5, then the own camera turned about its y axis and
    shifted sideways a little more each time (numpy float64 products: any finite affine transform will do)."""
    cams = list(vk.cameras(name))[:n]
    T0 = vk.cameras(name)[0].transform
    for k in range(len(cams), n):
        a = 0.004 * (k - 64)
        rot = np.array([[np.cos(a), 0, np.sin(a), 0], [0, 1, 0, 0], [-np.sin(a), 0, np.cos(a), 0], [0, 0, 0, 1]])
        shift = np.eye(4)
        shift[0, 3], shift[1, 3] = 0.01 * (k % 7 - 3), 0.005 * (k % 5 - 2)
        cams.append(vk.cameras(name)[k % 5].replace(transform=T0 @ shift @ rot))
    return cams


def _depth0_blob(name):
    blob = bytearray(pyoracle.golden_scene(name))
    nsec = struct.unpack_from("<I", blob, 8)[0]
    for i in range(nsec):
        tag, _, off, _ = struct.unpack_from("<IIQQ", blob, 16 + 24 * i)
        if tag == 0x52444E52:  # 'RNDR': maxRecursionDepth 0 (jsrt_params.max_depth 0 means "the blob's")
            struct.pack_into("<I", blob, off + 8, 0)
    return bytes(blob)


SHAPES = {  # case -> (W, H, views, spp, max_paths, depth: None = the scene's)
    "7x9x1": (7, 9, 1, 2, 0, None), "7x9x3": (7, 9, 3, 2, 0, None), "7x9x65": (7, 9, 65, 2, 0, None),
    "1x1x130": (1, 1, 130, 2, 0, None), "13x7x3_chunks": (13, 7, 3, 3, 128, None), "depth16": (7, 9, 1, 2, 0, 16)}


@pytest.mark.parametrize("case", sorted(SHAPES))
@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("name", ["cornell_box_path", "Aggregates"])
def test_view_shapes_against_the_oracle(jr, name, kind, case):
    W, H, nv, spp, max_paths, depth = SHAPES[case]
    depth = depth or vk.load(name)["depth"]
    spp = 1 if kind == 0 else spp
    cams = _many_cameras(name, nv)
    st = {}
    rgba, colors = _scene(jr, name).render_views(cams, W, H, spp, depth, kind, 9, max_paths=max_paths, want_colors=True,
                                                 stats=st)
    assert rgba.shape == (nv, H, W, 4) and st["samples"] == nv * W * H * spp
    if max_paths and kind:
        # 273 items in ranges of 128 (the first ends inside view 1, the second inside view 2), one sample per chunk
        assert st["batches"] >= 9
    for v in range(nv):
        orgba, ocol = _oracle_view(name, cams[v], W, H, spp, depth, kind, 9, key=(name, v, W, H, spp, depth, kind))
        _compare(rgba[v], colors[v], orgba, ocol, f"{name} {case} kind {kind} view {v}")
    if nv > 1 and (W, H) != (1, 1):
        assert (rgba[0] != rgba[1]).any()


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("name", ["cornell_box_path", "Aggregates"])
def test_depth_zero_is_black(jr, name, kind):
    blob0 = _depth0_blob(name)
    sc = jr.Scene(blob0, device=0)
    st = {}
    rgba, colors = sc.render_views(_many_cameras(name, 3), 7, 9, 2, 0, kind, 9, want_colors=True, stats=st)
    assert (rgba == np.array([0, 0, 0, 255], np.uint8)).all()
    assert np.array_equal(_bits(colors), _bits(np.broadcast_to(np.array([0, 0, 0, 1], np.float32), colors.shape)))
    assert st["batches"] == 0  # nothing is traced
    own_rgba, own_col, _ = sc.render(7, 9, 2, 0, kind, 9)
    assert _same(rgba[0], colors[0], own_rgba, own_col)
    ocol, orgba, _ = pyoracle.render(blob0, 7, 9, 2, 0, kind, 9)
    assert np.array_equal(orgba, rgba[1]) and np.array_equal(_bits(ocol[..., :3]), _bits(colors[1][..., :3]))


# ---- 5. independence ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_box_path", "bunny"])
def test_a_view_depends_on_its_camera_alone(jr, monkeypatch, name):
    k = vk.load(name)
    args = (k["width"], k["height"], k["spp"], k["depth"], k["kind"], k["seed"])
    cams = vk.cameras(name)
    sc = _scene(jr, name)
    one = {}
    rgba, colors = sc.render_views(cams, *args, want_colors=True, stats=one)
    for v in range(5):  # nviews 1 against 5, and the view's place in the call
        r1, c1 = sc.render_views([cams[v]], *args, want_colors=True)
        assert _same(r1[0], c1[0], rgba[v], colors[v]), f"{name}: view {v} alone differs"
    rr, cr = sc.render_views(cams[::-1], *args, want_colors=True)
    assert _same(rr[::-1], cr[::-1], rgba, colors)
    st = {}
    rm, cm = sc.render_views(cams, *args, max_paths=448, want_colors=True, stats=st)  # 1200 items: 3 ranges, mid-view
    assert st["batches"] >= 3 and one["batches"] < st["batches"]
    assert _same(rm, cm, rgba, colors), f"{name}: max_paths changes a view"
    monkeypatch.setenv("JSRT_HYBRID", "0" if name == "cornell_box_path" else "1")  # the other schedule
    ro, co = jr.Scene(pyoracle.golden_scene(name), device=0).render_views(cams, *args, want_colors=True)
    assert _same(ro, co, rgba, colors), f"{name}: the schedule changes a view"


# ---- 6. view_seeds ------------------------------------------------------------------------------------------------
def test_view_seeds(jr):
    name = "cornell_box_path"
    k = vk.load(name)
    W, H, spp, depth, kind = k["width"], k["height"], k["spp"], k["depth"], k["kind"]
    cams = vk.cameras(name)
    sc = _scene(jr, name)
    seeds = [11, 12, 13, 0xFFFFFFFF, 11]
    rgba, colors = sc.render_views(cams, W, H, spp, depth, kind, seed=99, view_seeds=seeds, want_colors=True)
    for v, s in enumerate(seeds):
        assert _same(rgba[v], colors[v], *_solo_render(jr, name, v, W, H, spp, depth, kind, s)), f"view {v} seed {s}"
    # the same camera under two seeds gives two images; no seeds: the call's seed for every view
    r2, c2 = sc.render_views([cams[0], cams[0]], W, H, spp, depth, kind, view_seeds=[11, 12], want_colors=True)
    assert _same(r2[0], c2[0], rgba[0], colors[0]) and (r2[0] != r2[1]).any()
    r3, c3 = sc.render_views(cams, W, H, spp, depth, kind, seed=11, want_colors=True)
    for v in range(5):
        assert _same(r3[v], c3[v], *_solo_render(jr, name, v, W, H, spp, depth, kind, 11))
    with pytest.raises(jr.JsrtError, match="one seed per camera"):
        sc.render_views(cams, W, H, view_seeds=[1, 2])


# ---- 7. the device entry ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_box_path", "bunny", "SDF_Menger"])
def test_device_entry_and_renders_left_alone(jr, name):
    import torch
    k = vk.load(name)
    args = (k["width"], k["height"], k["spp"], k["depth"], k["kind"], k["seed"])
    cams = vk.cameras(name)
    sc = _scene(jr, name)
    before = sc.render(24, 16, 2, 0, 1, 7)
    host = sc.render_views(cams, *args, want_colors=True)
    stream = torch.cuda.Stream(device=0)
    with torch.cuda.stream(stream):
        t_rgba, t_col = sc.render_views(cams, *args, want_colors=True, device=True)
        only = sc.render_views(cams, *args, device=True)
    stream.synchronize()
    assert isinstance(t_rgba, torch.Tensor) and t_rgba.is_cuda and t_rgba.dtype == torch.uint8 and t_col.dtype == torch.float32
    assert tuple(t_rgba.shape) == host[0].shape and tuple(t_col.shape) == host[1].shape
    assert _same(t_rgba.cpu().numpy(), t_col.cpu().numpy(), *host)
    assert np.array_equal(only.cpu().numpy(), host[0])
    after = sc.render(24, 16, 2, 0, 1, 7)
    assert _same(before[0], before[1], after[0], after[1])


# ---- 8. refusals --------------------------------------------------------------------------------------------------
def test_refused_arguments(jr):
    from jsraytracer_amd import _native
    L = _native.views_api()
    sc = _scene(jr, "BoxBall_path")
    cams = vk.cameras("BoxBall_path")
    recs = (_native.CameraRec * 2)(cams[0]._rec(), cams[1]._rec())
    out = np.zeros((2, 12, 20, 4), np.uint8)

    def call(p, c=recs, n=2, o=out.ctypes.data):
        return L.jsrt_render_views(sc._h, ctypes.byref(p), c, n, None, o, None, None)

    def bad(recs2=None, n=2, o=out.ctypes.data, **kw):
        p = sc.params(20, 12, 1, 0, 1, 1, device=0, **kw)
        rc = call(p, recs2 or recs, n, o)
        msg = _native.last_error()
        if rc == -1:  # the device entry refuses the same arguments the same way (before its pointers are used)
            assert L.jsrt_render_views_device(sc._h, ctypes.byref(p), recs2 or recs, n, None, o, None, None, None) == -1
            assert _native.last_error() == msg
        return rc, msg

    assert bad()[0] == 0 and out.any()  # the good call
    for kw, field in (({"x_offset": 1}, "x_offset"), ({"x_delt": 2}, "x_delt"), ({"device_mask": 2}, "device_mask"),
                      ({"mode": 1}, "mode")):
        rc, msg = bad(**kw)
        assert rc == -1 and msg.startswith(field), (kw, msg)
    assert bad(device_mask=1)[0] == 0  # the scene's own device
    assert bad(x_delt=1)[0] == 0 and bad(x_delt=0)[0] == 0
    for n in (0, -3):
        rc, msg = bad(n=n)
        assert rc == -1 and "nviews" in msg
    p = sc.params(1 << 15, 1 << 15, 1, 0, 1, 1, device=0)  # one view is 2^30 pixels, two are 2^31
    assert call(p, recs, 2) == -1 and "nviews * width * height" in _native.last_error()
    skew = cams[1].replace(transform=cams[1].transform + np.array([[0] * 4] * 3 + [[0, 0, 0.5, 0]]))
    rc, msg = bad((_native.CameraRec * 2)(cams[0]._rec(), skew._rec()))
    assert rc == -1 and "non-affine camera transform" in msg and "cams[1]" in msg
    for kind in (2, -1):
        rc, msg = bad((_native.CameraRec * 2)(cams[0].replace(kind=kind)._rec(), cams[1]._rec()))
        assert rc == -1 and msg.startswith("cams[0].kind"), msg
    rc, msg = bad(o=None)
    assert rc == -1 and "rgba8 is NULL" in msg
    assert call(sc.params(20, 12, 1, 0, 1, 1, device=0), None, 2) == -1 and _native.last_error() == "cams is NULL"
    assert L.jsrt_scene_camera(sc._h, None) == -1 and L.jsrt_scene_camera(None, ctypes.byref(recs[0])) == -1
    with pytest.raises(jr.JsrtError, match="nviews"):
        sc.render_views([])
