"""The arms of the frame planner and of the schedule that no default thumbnail reaches, each forced by its knob on a
thumbnail whose last 8 x 8 patches are partial.  Bar (test_gpu_parity): RGBA8 identical to the oracle, the same
NaN/inf pattern, |dRGB| <= 1e-5, stats["samples"] exact; and, each case being a knob variant of a default render,
bit for bit the default render of a fresh Scene (rgba and the u32 view of colors).

Split frame (plan_batches' halves, JSRT_SPLIT_MIN=8: from 256 paths): cornell_box_path spp 5 (sample-major: 3 + 2
samples); bunny 36 x 20 spp 3 (pixel-major, 15 patches: pixel halves of 8 and 7 patches), the same with
JSRT_SPLIT_PIXELS=0 (2 + 1 samples), JSRT_SPLIT_FRAME=0 (one batch) and JSRT_TILE_PATCHES=2 (the halves cut
through tiles); refraction_path with JSRT_BOUND_MARGIN=0.5 (the second half outgrows the bounds learned from the
first: the redo of a split frame on two pools).
Forced schedules, plain and over >= 3 batches: JSRT_HYBRID=0 on the analytic profile (run_batch<PF_ANALYTIC,false>:
k_shade<PF_ANALYTIC,false,true>, k_shadow<PF_ANALYTIC,false,...> / k_shadow_node<PF_ANALYTIC,false,4> with grid
buckets); JSRT_HYBRID=1 on BVH, aggregate and SDF scenes (run_batch<PF_MESH|PF_ALL|PF_SDF,true> with W.hybrid);
JSRT_POOL_FACTOR=1 on one of each (the tree's pool and the side-chain slots overflow: attempts >= 2).
SDF: JSRT_PERSIST=0 (plain k_extend<PF_SDF,...> and bucketed k_shadow<PF_SDF,...>), JSRT_SDF_FO=0 (the VM fallback
inside the persistent march; read when the scene is created), JSRT_SPLIT=0 (k_shadow on the batch stream),
JSRT_DUAL=1 (persistent casts on two streams).
Hand-off keys: JSRT_BUCKET_GRID=0 on cornell_box_path (primitive buckets on the flat profile, under both
JSRT_SHADOW_NODE settings), JSRT_CHILD_SORT=1 with JSRT_HYBRID=0 on cornell_box_path, JSRT_CHILD_SORT=0 on bunny.
Knob hygiene: knobs set to an empty string render the default image.
Streams (test_gpu_redo_streams' harness: jsrt_render_device on a caller stream, the tile copied on that stream
at once, so completeness on return is what is checked): JSRT_SPLIT=1 (k_shadow on its own stream beside two batch
streams) and JSRT_DUAL=0 on cornell_box_path and bunny over >= 3 batches."""
import numpy as np
import pytest

from oracle import pyoracle

pytestmark = pytest.mark.gpu
TOL = 1e-5
S, L, ODD = (28, 20), (44, 36), (36, 20)  # ODD: 5 x 3 = 15 patches, so pixel halves of 8 and 7
SPLIT = {"JSRT_SPLIT_MIN": "8"}
MANY = {"max_paths": 1280}  # >= 3 batches of a 44 x 36 frame (1,920 patch pixels) in either path order


def _c(scene, size, spp, cap, seed, env, kw=None, **expect):
    return (scene, size, spp, cap, seed, env, kw or {}, expect)


CASES = [
    # split frame
    _c("cornell_box_path", S, 5, 6, 3, SPLIT, batches=2),
    _c("bunny", ODD, 3, 4, 4, SPLIT, batches=2),
    _c("bunny", ODD, 3, 4, 4, {**SPLIT, "JSRT_SPLIT_PIXELS": "0"}, batches=2),
    _c("bunny", ODD, 3, 4, 4, {**SPLIT, "JSRT_SPLIT_FRAME": "0"}, batches=1),
    _c("bunny", ODD, 3, 4, 4, {**SPLIT, "JSRT_TILE_PATCHES": "2"}, batches=2),
    _c("refraction_path", L, 3, 6, 5, {**SPLIT, "JSRT_BOUND_MARGIN": "0.5"}, batches=2, min_attempts=2),
    # forced schedules
    *[_c(n, sz, spp, 6, 6, {"JSRT_HYBRID": "0"}, kw, **ex)
      for n, spp in (("cornell_box_path", 3), ("refraction_path", 2), ("refraction", 5))
      for sz, kw, ex in ((S, {}, {}), (L, MANY, {"min_batches": 3}))],
    *[_c(n, sz, spp, 4, 7, {"JSRT_HYBRID": "1"}, kw, **ex)
      for n, spp in (("bunny", 3), ("Aggregates", 2), ("AMultipleBVH", 5), ("SDF_Combinations", 2), ("SDF_Menger", 3))
      for sz, kw, ex in ((S, {}, {}), (L, MANY, {"min_batches": 3}))],
    _c("cornell_box_path", L, 3, 6, 8, {"JSRT_HYBRID": "0", "JSRT_POOL_FACTOR": "1"}, min_attempts=2),
    _c("bunny", L, 3, 4, 8, {"JSRT_HYBRID": "1", "JSRT_POOL_FACTOR": "1"}, min_attempts=2),
    # SDF
    _c("SDF_Menger", S, 3, 4, 9, {"JSRT_PERSIST": "0"}),
    _c("SDF_Simple", L, 2, 4, 9, {"JSRT_PERSIST": "0"}),
    _c("SDF_Menger", S, 3, 4, 9, {"JSRT_SDF_FO": "0"}),
    _c("SDF_Sierpinski", L, 2, 4, 9, {"JSRT_SDF_FO": "0"}),
    _c("SDF_Menger", S, 3, 4, 9, {"JSRT_SPLIT": "0"}),
    _c("SDF_Menger", L, 3, 4, 9, {"JSRT_DUAL": "1"}, MANY, min_batches=3),
    # ... and the instantiations only two knobs together reach: the hybrid chain on an SDF scene without persistent
    # casts (k_extend<PF_SDF,true>, k_shadow<PF_SDF,true,...>) and with the VM fallback (k_extend_q<PF_SDF,true,false>,
    # k_shadow_cast<PF_SDF,true,false>); the tree with unstaged tables (k_shade<PF_ANALYTIC,false,false>,
    # k_shadow<PF_ANALYTIC,false,false,false,false>)
    _c("SDF_Menger", S, 3, 4, 9, {"JSRT_HYBRID": "1", "JSRT_PERSIST": "0"}),
    _c("SDF_Menger", S, 3, 4, 9, {"JSRT_HYBRID": "1", "JSRT_SDF_FO": "0"}),
    _c("cornell_box_path", L, 3, 6, 10, {"JSRT_HYBRID": "0", "JSRT_SHADE_LDS": "0"}),
    # hand-off keys
    _c("cornell_box_path", L, 3, 6, 10, {"JSRT_BUCKET_GRID": "0", "JSRT_SHADOW_NODE": "0"}),
    _c("cornell_box_path", L, 3, 6, 10, {"JSRT_BUCKET_GRID": "0", "JSRT_SHADOW_NODE": "1"}),
    _c("cornell_box_path", L, 3, 6, 10, {"JSRT_CHILD_SORT": "1", "JSRT_HYBRID": "0"}),
    _c("bunny", S, 5, 4, 10, {"JSRT_CHILD_SORT": "0"}),
    # knob hygiene
    _c("bunny", S, 5, 4, 10, {"JSRT_PIXEL_MAJOR": ""}),
    _c("cornell_box_path", L, 3, 6, 10, {k: "" for k in ("JSRT_PIXEL_MAJOR", "JSRT_DUAL", "JSRT_SPLIT", "JSRT_CHILD_SORT",
                                                          "JSRT_BUCKET_GRID", "JSRT_SHADOW_NODE", "JSRT_SHADOW_SERIAL")}),
]
STREAM_CASES = [(n, L, spp, cap, env) for n, spp, cap in (("cornell_box_path", 3, 6), ("bunny", 5, 4))
                for env in ({"JSRT_SPLIT": "1"}, {"JSRT_DUAL": "0"})]


def _env_id(env):
    return "+".join(f"{k[5:]}={v}" for k, v in env.items())


def _id(c):
    return f"{c[0]}_{c[1][0]}x{c[1][1]}_s{c[2]}_{_env_id(c[5])}" + ("_many" if c[6] else "")


@pytest.fixture(scope="module")
def jr():
    import jsraytracer_amd as jr
    return jr


_oracle, _default = {}, {}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _reference(name, W, H, spp, depth, seed):
    key = (name, W, H, spp, depth, seed)
    if key not in _oracle:
        ocol, orgba, _ = pyoracle.render(pyoracle.golden_scene(name), W, H, spp, depth, 1, seed)
        _oracle[key] = _frozen(ocol, orgba)
    return _oracle[key]


def _default_render(jr, name, W, H, spp, depth, seed):
    """The frame with no knob set, on a fresh Scene (call before any setenv)."""
    key = (name, W, H, spp, depth, seed)
    if key not in _default:
        rgba, colors, _ = jr.Scene(pyoracle.golden_scene(name), device=0).render(W, H, spp, depth, 1, seed)
        _default[key] = _frozen(rgba, colors)
    return _default[key]


def _compare(rgba, colors, grgba, gcol, label):
    bad = (rgba != grgba).any(-1)
    assert not bad.any(), f"{label}: {int(bad.sum())} RGBA8 pixels differ"
    fin = np.isfinite(gcol[..., :3])
    assert np.array_equal(np.isfinite(colors[..., :3]), fin), f"{label}: NaN/inf pattern differs"
    err = float(np.abs(colors[..., :3][fin] - gcol[..., :3][fin]).max()) if fin.any() else 0.0
    assert err <= TOL, f"{label}: max |dRGB| {err}"


def _expect(st, expect, label):
    print(f"{label}: batches {st['batches']} attempts {st['attempts']}")
    if "batches" in expect:
        assert st["batches"] == expect["batches"], label
    if "min_batches" in expect:
        assert st["batches"] >= expect["min_batches"], label
    if "min_attempts" in expect:
        assert st["attempts"] >= expect["min_attempts"], label


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_schedule_arm_matches_oracle_and_default(jr, monkeypatch, case):
    name, (W, H), spp, cap, seed, env, kw, expect = case
    blob = pyoracle.golden_scene(name)
    depth = min(cap, pyoracle.scene_header(blob)["max_depth"])
    ocol, orgba = _reference(name, W, H, spp, depth, seed)
    rgba0, col0 = _default_render(jr, name, W, H, spp, depth, seed)
    _compare(rgba0, col0, orgba, ocol, f"{name} default")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rgba, colors, st = jr.Scene(blob, device=0).render(W, H, spp, depth, 1, seed, **kw)
    _compare(rgba, colors, orgba, ocol, _id(case))
    assert st["samples"] == W * H * spp
    assert np.array_equal(rgba, rgba0)
    assert np.array_equal(colors.view(np.uint32), col0.view(np.uint32))
    _expect(st, expect, _id(case))


@pytest.mark.parametrize("case", STREAM_CASES, ids=lambda c: f"{c[0]}_{_env_id(c[4])}")
def test_device_frame_complete_on_return(jr, monkeypatch, case):
    torch = pytest.importorskip("torch")
    name, (W, H), spp, cap, env = case
    blob = pyoracle.golden_scene(name)
    depth = min(cap, pyoracle.scene_header(blob)["max_depth"])
    _, orgba = _reference(name, W, H, spp, depth, 3)
    rgba0, _ = _default_render(jr, name, W, H, spp, depth, 3)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc = jr.Scene(blob, device=0)
    stream = torch.cuda.Stream()
    tile = torch.zeros(W * H, dtype=torch.int32, device="cuda:0")
    kw = dict(width=W, height=H, spp=spp, max_depth=depth, kind=1, seed=3, **MANY)
    with torch.cuda.stream(stream):
        tile.fill_(-1)  # (a pixel the frame never wrote reads as 0xFFFFFFFF)
        # stats=False: the call returns without waiting for the device (stats would synchronise the stream)
        sc.render_device(tile.data_ptr(), stream_ptr=stream.cuda_stream, stats=False, **kw)
        got = tile.clone()  # enqueued on the render's stream right behind it
    stream.synchronize()
    img = got.cpu().numpy().view(np.uint8).reshape(W, H, 4).transpose(1, 0, 2)  # [owned column][row] -> [row][col]
    bad = (img != orgba).any(-1)
    assert not bad.any(), f"{name} {env}: {int(bad.sum())} of {bad.size} pixels differ"
    assert np.array_equal(img, rgba0)
    st = jr.Scene(blob, device=0).render_device(tile.data_ptr(), stream_ptr=stream.cuda_stream, **kw)
    assert st["batches"] >= 3
