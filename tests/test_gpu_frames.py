"""Frames at the recursion depths and frame shapes no other GPU test renders: maxRecursionDepth 1 ... 3 and 9 ... 16
(the library accepts 1 ... MAX_TREE_DEPTH = 16, every other test renders at 4 ... 8) and frames that are no multiple of
the 8 x 8 patch -- one pixel, one row, one column, primes, narrower than a wave -- in all three renderer kinds.

Bar (BASELINE north star, test_gpu_parity._compare): RGBA8 identical, the same NaN/inf pattern, |dRGB| <= 1e-5,
stats["samples"] exact.  The count of f32 values that are not bit-identical is printed per case.

  1. every golden of tests/golden/frames/ (the reference's own frames, oracle/refharness/regen_frames.sh) through
     Scene.render;
  2. depth x schedule against the oracle (pinned to those goldens by test_oracle_frames.py) at 20 x 12, spp 2, seed 3:
     depths 1, 2, 9, 16 on cornell_box_path, refraction_path (hybrid chain by default), bunny and diamond (tree by
     default), each under the default schedule, the other one (JSRT_HYBRID=0 / 1: the tree at depth 16, the hybrid
     side chains of two-child materials at depth 16, resolve_chain's direct node load above 8 levels) and a max_paths
     that cuts the frame into >= 3 batches; every knob case equals the default render of a fresh Scene bit for bit.
     One depth-16 frame under JSRT_POOL_FACTOR=1 is redone (attempts >= 2) and does not change;
  3. World.color at depth 16: Scene.color over Scene.camera_rays, accumulated per sample, is the render;
  4. shape x kind x profile against the oracle: (1,1), (1,7), (13,1), (7,9), (37,23), (9,65) x kinds 0, 1, 2 x
     cornell_box_path (analytic), bunny (mesh), SDF_Menger (SDF), Aggregates (all); the two large ones also with
     JSRT_SPLIT_MIN=8, where the halves of a split frame cut through partial patches;
  5. partition edges: four workers' columns of kinds 0 and 2 composite to the frame; x_delt = W (a column per
     worker); x_offset >= W (nothing owned: the call succeeds and touches nothing); block-cyclic device tiles whose
     last block is partial, and ranks that own nothing;
  6. limits: depth 17 is refused, 16 accepted."""
import numpy as np
import pytest

from oracle import pyoracle

pytestmark = pytest.mark.gpu
TOL = 1e-5
SUB = "frames"
RENDERS = pyoracle.golden_index(SUB)
LW, LH, LSPP, LSEED = 20, 12, 2, 3  # the depth ladder's frame (tests/golden/frames, test_oracle_frames.py)


@pytest.fixture(scope="module")
def jr():
    import jsraytracer_amd as jr
    return jr


_scenes, _oracle, _default = {}, {}, {}


def _scene(jr, name):
    if name not in _scenes:
        _scenes[name] = jr.Scene(pyoracle.golden_scene(name), device=0)
    return _scenes[name]


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _reference(name, W, H, spp, depth, kind, seed, x_offset=0, x_delt=1):
    """The oracle's (colors, rgba) of a frame: computed once, shared, read-only."""
    key = (name, W, H, spp, depth, kind, seed, x_offset, x_delt)
    if key not in _oracle:
        ocol, orgba, _ = pyoracle.render(pyoracle.golden_scene(name), *key[1:])
        _oracle[key] = _frozen(ocol, orgba)
    return _oracle[key]


def _default_render(jr, name, W, H, spp, depth, kind, seed):
    """The frame with no knob set, on a fresh Scene (call before any setenv): (rgba, colors), computed once."""
    key = (name, W, H, spp, depth, kind, seed)
    if key not in _default:
        rgba, colors, st = jr.Scene(pyoracle.golden_scene(name), device=0).render(W, H, spp, depth, kind, seed)
        assert st["samples"] == W * H * (spp if kind else 1)
        _default[key] = _frozen(rgba, colors)
    return _default[key]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_frame(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))


def _compare(rgba, colors, grgba, gcol, label):
    got, want = colors[..., :3], gcol[..., :3]
    notbit = int(((_bits(got) != _bits(want)) & ~(np.isnan(got) & np.isnan(want))).sum())
    fin = np.isfinite(want)
    err = float(np.abs(got[fin] - want[fin]).max()) if fin.any() and np.isfinite(got[fin]).all() else 0.0
    print(f"{label}: {notbit} of {want.size} f32 values not bit-identical, max |dRGB| = {err:.3g}")
    bad = (rgba != grgba).any(-1)
    assert not bad.any(), f"{label}: {int(bad.sum())} RGBA8 pixels differ, max {int(np.abs(rgba.astype(int) - grgba).max())}"
    assert np.array_equal(np.isfinite(got), fin), f"{label}: NaN/inf pattern differs"
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{label}: NaN pattern differs"
    assert err <= TOL, f"{label}: max |dRGB| {err}"


def _owned(W, x_offset, x_delt):
    return list(range(x_offset, W, x_delt))


# ---- 1. the reference's frames ----------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", sorted(RENDERS))
def test_gpu_matches_reference_frame(jr, tag):
    r = RENDERS[tag]
    W, H = r["width"], r["height"]
    rgba, colors, st = _scene(jr, r["scene"]).render(W, H, r["spp"], r["depth"], r["kind"], r["seed"], r["x_offset"],
                                                     r["x_delt"])
    gcol, grgba = pyoracle.golden_image(tag, W, H, sub=SUB)
    cols = _owned(W, r["x_offset"], r["x_delt"])
    assert st["samples"] == len(cols) * H * r["spp"]  # (a kind-0 golden has spp 1)
    assert st["attempts"] >= 1 and st["batches"] >= 1
    assert not np.delete(rgba, cols, axis=1).any()  # untouched columns stay zero (worker.js: a fresh ImageData)
    assert np.isnan(np.delete(colors, cols, axis=1)).all()
    _compare(rgba[:, cols], colors[:, cols], grgba[:, cols], gcol[:, cols], tag)


# ---- 2. depth x schedule ----------------------------------------------------------------------------------------
DEPTHS = (1, 2, 9, 16)
ANALYTIC, MESH = ("cornell_box_path", "refraction_path"), ("bunny", "diamond")
MANY = 128  # max_paths: the 6 patches (384 patch pixels) x 2 samples in batches of 128 paths (2 patches x 1 sample, or
#             pixel-major 1 patch x 2 samples): 6 batches in either path order
ARMS = ("default", "other", "many")


@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("name", ANALYTIC + MESH)
def test_depth_under_each_schedule(jr, monkeypatch, name, depth, arm):
    label = f"{name} depth {depth} {arm}"
    ocol, orgba = _reference(name, LW, LH, LSPP, depth, 1, LSEED)
    rgba0, col0 = _default_render(jr, name, LW, LH, LSPP, depth, 1, LSEED)
    if arm == "default":
        _compare(rgba0, col0, orgba, ocol, label)
        return
    kw = {}
    if arm == "other":
        monkeypatch.setenv("JSRT_HYBRID", "0" if name in ANALYTIC else "1")
    else:
        kw["max_paths"] = MANY
    rgba, colors, st = jr.Scene(pyoracle.golden_scene(name), device=0).render(LW, LH, LSPP, depth, 1, LSEED, **kw)
    print(f"{label}: batches {st['batches']} attempts {st['attempts']}")
    _compare(rgba, colors, orgba, ocol, label)
    assert st["samples"] == LW * LH * LSPP and st["attempts"] >= 1
    if arm == "many":
        assert st["batches"] >= 3, label
    assert _same_frame((rgba, colors), (rgba0, col0)), f"{label}: differs from the default render"


def test_depth_16_pool_overflow_is_redone(jr, monkeypatch):
    """refraction_path at depth 16 starts far more side chains than JSRT_POOL_FACTOR=1 leaves slots for (a quarter of
    the paths): the frame is poisoned, redone with a doubled pool until it fits, and comes back unchanged."""
    name = "refraction_path"
    ocol, orgba = _reference(name, LW, LH, LSPP, 16, 1, LSEED)
    rgba0, col0 = _default_render(jr, name, LW, LH, LSPP, 16, 1, LSEED)
    monkeypatch.setenv("JSRT_POOL_FACTOR", "1")
    rgba, colors, st = jr.Scene(pyoracle.golden_scene(name), device=0).render(LW, LH, LSPP, 16, 1, LSEED)
    print(f"{name} depth 16 POOL_FACTOR=1: batches {st['batches']} attempts {st['attempts']}")
    _compare(rgba, colors, orgba, ocol, f"{name} depth 16 POOL_FACTOR=1")
    assert st["samples"] == LW * LH * LSPP and st["attempts"] >= 2
    assert _same_frame((rgba, colors), (rgba0, col0))


# ---- 3. World.color at depth ------------------------------------------------------------------------------------
def _accumulate(kind, samples):
    """The renderer's f32 accumulation of a pixel's samples in order and its final colour (renderers.js:52-61 Random,
    :93-98 Incremental; render_levels.h accumulate, render.hip k_final), as in test_gpu_color.py."""
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


@pytest.mark.parametrize("name", ["cornell_box_path", "bunny"])
def test_color_of_camera_rays_is_the_render_at_depth_16(jr, name):
    sc = _scene(jr, name)
    keys = np.arange(LW * LH, dtype=np.uint32)
    samples = []
    for s in range(LSPP):
        rays = sc.camera_rays(LW, LH, kind=1, seed=LSEED, sample=s)
        assert rays.shape == (LW * LH, 6) and np.isfinite(rays).all()
        samples.append(sc.color(rays, keys, max_depth=16, seed=LSEED, sample0=s)[:, 0])
    mine = _accumulate(1, samples)
    _, colors, _ = sc.render(LW, LH, LSPP, 16, 1, LSEED)
    ocol, _ = _reference(name, LW, LH, LSPP, 16, 1, LSEED)
    assert np.array_equal(_bits(mine), _bits(colors[..., :3].reshape(-1, 3))), "differs from jsrt_render's colors_f32"
    assert np.array_equal(_bits(mine), _bits(ocol[..., :3].reshape(-1, 3))), "differs from the oracle's colours"
    # ... and level 15 is live in it: one level less is another frame
    shallow = _accumulate(1, [sc.color(sc.camera_rays(LW, LH, kind=1, seed=LSEED, sample=s), keys, max_depth=15,
                                       seed=LSEED, sample0=s)[:, 0] for s in range(LSPP)])
    assert not np.array_equal(_bits(mine), _bits(shallow))


# ---- 4. shape x kind x profile ----------------------------------------------------------------------------------
SIZES = [(1, 1), (1, 7), (13, 1), (7, 9), (37, 23), (9, 65)]
SHAPE_SCENES = ["cornell_box_path", "bunny", "SDF_Menger", "Aggregates"]  # PF_ANALYTIC, PF_MESH, PF_SDF, PF_ALL
SSEED = 3
_plain = {}


def _shape_case(name, kind):
    return (3 if kind else 1), pyoracle.scene_header(pyoracle.golden_scene(name))["max_depth"]


def _plain_render(jr, name, W, H, kind):
    key = (name, W, H, kind)
    if key not in _plain:
        spp, depth = _shape_case(name, kind)
        rgba, colors, st = _scene(jr, name).render(W, H, spp, depth, kind, SSEED)
        _plain[key] = (*_frozen(rgba, colors), st)
    return _plain[key]


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", SHAPE_SCENES)
def test_shape_kind_profile(jr, name, size, kind):
    W, H = size
    spp, depth = _shape_case(name, kind)
    ocol, orgba = _reference(name, W, H, spp, depth, kind, SSEED)
    rgba, colors, st = _plain_render(jr, name, W, H, kind)
    assert rgba.shape == (H, W, 4) and colors.shape == (H, W, 4)
    _compare(rgba, colors, orgba, ocol, f"{name} {W}x{H} kind {kind}")
    assert st["samples"] == W * H * spp
    assert (rgba[..., 3] == 255).all()  # every pixel of the frame was written


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("size", [(37, 23), (9, 65)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", SHAPE_SCENES)
def test_shape_split_frame(jr, monkeypatch, name, size, kind):
    """JSRT_SPLIT_MIN=8: a frame of 2^8 paths or more that fits one batch is cut into two (plan_batches).  15 and 18
    patches: pixel halves of 8 + 7 and 9 + 9 patches (pixel-major profiles), sample halves of 2 + 1 (cornell), all
    over partial last patches.  A kind-0 frame (one sample) and a frame with persistent SDF casts (SDF_Menger) stay
    one batch; they must not change either."""
    W, H = size
    spp, depth = _shape_case(name, kind)
    ocol, orgba = _reference(name, W, H, spp, depth, kind, SSEED)
    rgba0, col0, _ = _plain_render(jr, name, W, H, kind)
    monkeypatch.setenv("JSRT_SPLIT_MIN", "8")
    rgba, colors, st = jr.Scene(pyoracle.golden_scene(name), device=0).render(W, H, spp, depth, kind, SSEED)
    label = f"{name} {W}x{H} kind {kind} SPLIT_MIN=8"
    print(f"{label}: batches {st['batches']} attempts {st['attempts']}")
    _compare(rgba, colors, orgba, ocol, label)
    assert st["samples"] == W * H * spp
    assert st["batches"] == (2 if kind and name != "SDF_Menger" else 1), label
    assert _same_frame((rgba, colors), (rgba0, col0)), f"{label}: differs from the unsplit render"


# ---- 5. partition edges -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 2])
def test_partition_invariance_simple_and_random(jr, kind):
    """renderers.js:88 column interleave in SimpleRenderer / RandomMultisamplingRenderer: four workers' images of a
    37 x 23 frame (10, 9, 9, 9 columns) composite to the single-worker frame, which is the oracle's."""
    W, H = 37, 23
    spp, depth = _shape_case("cornell_box_path", kind)
    sc = _scene(jr, "cornell_box_path")
    full, fcol, _ = _plain_render(jr, "cornell_box_path", W, H, kind)
    ocol, orgba = _reference("cornell_box_path", W, H, spp, depth, kind, SSEED)
    _compare(full, fcol, orgba, ocol, f"cornell_box_path 37x23 kind {kind}")
    comp, ccol = np.zeros_like(full), np.full_like(fcol, np.nan)
    for k in range(4):
        part, pcol, st = sc.render(W, H, spp, depth, kind, SSEED, k, 4)
        cols = _owned(W, k, 4)
        assert st["samples"] == len(cols) * H * spp
        assert not np.delete(part, cols, axis=1).any() and np.isnan(np.delete(pcol, cols, axis=1)).all()
        comp[:, cols], ccol[:, cols] = part[:, cols], pcol[:, cols]
    assert _same_frame((comp, ccol), (full, fcol))


def test_partition_one_column_per_worker(jr):
    """x_delt = W: worker k owns column k alone (a frame one pixel wide inside a 13-wide image)."""
    W, H, spp, depth = 13, 7, 2, 8
    sc = _scene(jr, "cornell_box_path")
    ocol, orgba = _reference("cornell_box_path", W, H, spp, depth, 1, SSEED)
    comp, ccol = np.zeros((H, W, 4), np.uint8), np.full((H, W, 4), np.nan, np.float32)
    for k in range(W):
        part, pcol, st = sc.render(W, H, spp, depth, 1, SSEED, k, W)
        assert st["samples"] == H * spp
        assert not np.delete(part, k, axis=1).any() and np.isnan(np.delete(pcol, k, axis=1)).all()
        comp[:, k], ccol[:, k] = part[:, k], pcol[:, k]
    _compare(comp, ccol, orgba, ocol, "cornell_box_path 13x7, a column per worker")


@pytest.mark.parametrize("x_offset", [13, 14, 40])
def test_partition_offset_past_the_frame_owns_nothing(jr, x_offset):
    """renderers.js:88 `for (px = x_offset; px < width; ...)`: a worker whose first column lies past the image
    renders nothing.  jsrt_render returns 0, leaves both buffers as they were and reports no samples."""
    W, H = 13, 7
    rgba = np.full((H, W, 4), 0xAB, np.uint8)
    got, colors, st = _scene(jr, "cornell_box_path").render(W, H, 2, 8, 1, SSEED, x_offset, 3, rgba=rgba)
    assert got is rgba and (rgba == 0xAB).all() and np.isnan(colors).all()
    assert st["samples"] == 0
    assert jr.owned_columns(W, x_offset, 3) == 0


@pytest.mark.parametrize("W,owned", [(37, (16, 13, 8)), (5, (5, 0, 0))])
def test_device_tiles_partial_last_block_and_empty_ranks(jr, W, owned):
    """jsrt_render_device over 3 ranks with col_block = 8.  W = 37: blocks 0 ... 4, the last one 5 columns wide
    (rank 1 owns 8 + 5).  W = 5: one partial block, ranks 1 and 2 own nothing -- the call succeeds and writes
    nothing into the tile a rank of the multi-GPU layout holds (sized for the widest rank)."""
    torch = pytest.importorskip("torch")
    H, spp, depth = 23, 2, 8
    sc = _scene(jr, "cornell_box_path")
    ocol, orgba = _reference("cornell_box_path", W, H, spp, depth, 1, SSEED)
    full, fcol, _ = sc.render(W, H, spp, depth, 1, SSEED)
    _compare(full, fcol, orgba, ocol, f"cornell_box_path {W}x{H}")
    comp = np.zeros_like(full)
    maxcols = max(owned)
    for r in range(3):
        nc = jr.owned_columns(W, r, 3, 8)
        assert nc == owned[r]
        d = torch.full((maxcols * H,), -1, dtype=torch.int32, device="cuda:0")
        st = sc.render_device(d.data_ptr(), col_block=8, width=W, height=H, spp=spp, max_depth=depth, kind=1, seed=SSEED,
                              x_offset=r, x_delt=3)
        torch.cuda.synchronize()
        assert st["samples"] == nc * H * spp
        got = d.cpu().numpy()
        assert (got[nc * H:] == -1).all()  # nothing past the rank's own columns
        cols = [c for c in range(W) if (c // 8) % 3 == r]
        assert len(cols) == nc
        comp[:, cols] = got[:nc * H].view(np.uint8).reshape(nc, H, 4).transpose(1, 0, 2)
    assert np.array_equal(comp, full)


# ---- 6. limits --------------------------------------------------------------------------------------------------
def test_depth_limit_through_render(jr):
    sc = _scene(jr, "cornell_box_path")
    with pytest.raises(jr.JsrtError, match="maxRecursionDepth above 16 is not supported"):
        sc.render(8, 8, 1, 17, 1, 1)
    rgba, colors, st = sc.render(1, 1, 1, 16, 1, 1)
    ocol, orgba = _reference("cornell_box_path", 1, 1, 1, 16, 1, 1)
    _compare(rgba, colors, orgba, ocol, "cornell_box_path 1x1 depth 16")
    assert st["samples"] == 1
