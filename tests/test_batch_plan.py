"""The frame planner (jsraytracer_amd/csrc/render_plan.h: plan_batches, the batch enumeration render_frame walks
-- batch_rows / batch_cols / batch_span --, two_full and pixel_of), compiled for the host: pure arithmetic that
only whole images checked so far.

Over the cross product of patches, spp, max_paths, ns, samples_per_batch, both profiles' pixel-major defaults,
JSRT_BATCH_SPP, JSRT_SPLIT_MIN, JSRT_SPLIT_PIXELS and JSRT_PERSIST (653,184 frames):
  * every (pixel, sample) of npix_total x spp lies in exactly one batch: the batches are rows of consecutive pixel
    spans, rows of consecutive samples (so a pixel's samples also reach the accumulation in order), and for
    frames of up to 2^14 pairs every pair is counted, too;
  * every batch has npix a non-zero multiple of 64 and nb >= 1;
  * no batch exceeds max(64, max_paths rescaled by 4 / ns for ns > 4) paths (the halves of a split frame are
    smaller than the one batch they were cut from, so they need no exception);
  * a frame is split exactly when the unsplit plan (JSRT_SPLIT_FRAME=0) is one batch of 2^split_min paths or more,
    without persistent casts and with spp >= 2; a split frame is exactly two batches that satisfy two_full (so
    they run on the two batch streams): pixel halves of ceil(patches / 2) and floor(patches / 2) patches from two
    patches on, else sample halves of (spp + 1) / 2 and spp / 2; any other frame equals its unsplit plan.
(The enumeration reads only the plan, the frame's pixels and spp, so it is walked once per distinct plan.)

pixel_of: for tile_p in {0, 1, 2, 3, 8} and every grid from 1 x 1 to 9 x 9 patches -- images that fill the last
patch row and column, and images that end 3 pixels into them -- the indices [0, npix_total) map one to one onto the
patch grid's pixels, valid exactly inside the image, with px the owned column's image column (round-robin and
block-cyclic column ownership)."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "batch_plan_host.hip")
OUT = os.path.join(ROOT, "tests", "native", "_build", "libbatch_plan_host.so")
HDRS = [os.path.join(ROOT, "jsraytracer_amd", "csrc", h) for h in ("render_plan.h", "render_kernel.h", "device_scene.h")]
PF_ANALYTIC, PF_SDF = 0, 4  # device_scene.h

PATCHES = [1, 2, 3, 25, 26, 127, 128, 129, 4096]
SPP = [1, 2, 3, 5, 64, 257]
MAX_PATHS = [1, 63, 64, 65, 640, 4096, 2**22, 2**25]
NS = [0, 1, 4, 5, 64, 65, 4096]
SAMPLES_PER_BATCH = [0, 1, 3]
PROFILES = [PF_ANALYTIC, PF_SDF]  # sample-major / pixel-major by default (JSRT_PIXEL_MAJOR unset)
BATCH_SPP = [1, 2, 256]
SPLIT_MIN = [1, 8, 22]
COUNT_CAP = 1 << 14


@pytest.fixture(scope="module")
def lib():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(f) for f in [SRC] + HDRS):
        subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-fno-fast-math", "-fPIC", "-shared", SRC, "-o", OUT + f".{os.getpid()}.tmp"], check=True)
        os.replace(OUT + f".{os.getpid()}.tmp", OUT)
    L = ctypes.CDLL(OUT)
    P, LL = ctypes.c_void_p, ctypes.c_longlong
    L.plan_many.argtypes = [LL, P, P]
    L.check_many.argtypes = [LL, P, P, LL, P, P, P]
    L.pixels.argtypes = [ctypes.c_int] * 7 + [P]
    return L


def _plans(lib, rows):
    rows = np.ascontiguousarray(rows, np.int64)
    out = np.empty((len(rows), 10), np.int64)
    lib.plan_many(len(rows), rows.ctypes.data, out.ctypes.data)
    return out


@pytest.fixture(scope="module")
def sweep(lib):
    """rows: one frame each {profile, all_roots_prims, patches, spp, samples_per_batch, ns, max_paths, pixel_major
    (-1: the profile's), batch_spp, tile_patches, persist, split_frame, split_min, split_pixels}; its plan; the plan
    of the same frame with JSRT_SPLIT_FRAME=0."""
    g = np.meshgrid(PROFILES, PATCHES, SPP, SAMPLES_PER_BATCH, NS, MAX_PATHS, BATCH_SPP, (0, 1), SPLIT_MIN, (0, 1), indexing="ij")
    pf, pa, spp, spb, ns, mp, bs, per, smin, sp = (x.reshape(-1).astype(np.int64) for x in g)
    one = np.ones_like(pf)
    rows = np.stack([pf, one, pa, spp, spb, ns, mp, -one, bs, 8 * one, per, one, smin, sp], 1)
    whole = rows.copy()
    whole[:, 11] = 0
    return rows, _plans(lib, rows), _plans(lib, whole)


def test_batches_cover_every_pixel_sample_once(lib, sweep):
    rows, plans, _ = sweep
    mp = rows[:, 6].copy()
    big = rows[:, 5] > 4
    mp[big] = mp[big] * 4 // rows[big, 5]
    limit = np.maximum(64, mp)
    keys, inverse = np.unique(np.concatenate([plans[:, :7], rows[:, 2:4]], 1), axis=0, return_inverse=True)
    keys = np.ascontiguousarray(keys)
    n = len(keys)
    codes, nb, maxp = np.empty(n, np.int32), np.empty(n, np.int64), np.empty(n, np.uint64)
    count = np.empty(COUNT_CAP, np.uint8)
    lib.check_many(n, keys.ctypes.data, count.ctypes.data, COUNT_CAP, codes.ctypes.data, nb.ctypes.data, maxp.ctypes.data)
    bad = np.flatnonzero(codes)
    assert bad.size == 0, f"check {codes[bad[0]]} fails for plan, patches, spp {keys[bad[0]]}"
    inverse = inverse.reshape(-1)
    assert (nb[inverse] == plans[:, 8] * plans[:, 9]).all()
    over = np.flatnonzero(maxp[inverse].astype(np.int64) > limit)
    assert over.size == 0, f"{rows[over[0]]}: a batch of {maxp[inverse][over[0]]} paths, limit {limit[over[0]]}"
    assert (keys[:, 7] * 64 * keys[:, 8] <= COUNT_CAP).sum() > 100  # frames whose pairs were counted one by one
    assert nb.max() >= 4096 * 257  # ... and frames of a batch per patch and sample


def test_split_frames_are_two_comparable_halves(sweep):
    rows, plans, whole = sweep
    patches, spp = rows[:, 2], rows[:, 3]
    total = patches * 64
    persist = (rows[:, 0] == PF_SDF) & (rows[:, 10] == 1)
    assert np.array_equal(plans[:, 4] == 1, persist)
    assert np.array_equal(plans[:, 2] == 1, rows[:, 0] != PF_ANALYTIC)  # the profiles' pixel-major defaults
    assert (whole[:, 6] == 0).all()
    fits = (whole[:, 0] == total) & (whole[:, 1] == spp)
    expect = fits & ~persist & (spp >= 2) & (total * spp >= (1 << rows[:, 12]))
    assert np.array_equal(plans[:, 6] == 1, expect)
    assert expect.sum() > 1000 and (~expect).sum() > 1000
    same = ~expect
    assert np.array_equal(plans[same], whole[same])  # no split: the unsplit plan, two_full and batch grid included
    s = plans[expect]
    assert (s[:, 8] * s[:, 9] == 2).all(), "a split frame is two batches"
    assert (s[:, 7] == 1).all(), "the halves of a split frame satisfy two_full"
    by_pixels = (plans[:, 2] == 1) & (rows[:, 13] == 1) & (patches >= 2)
    px, sm = expect & by_pixels, expect & ~by_pixels
    assert px.sum() > 100 and sm.sum() > 100
    assert np.array_equal(plans[px, 0], (patches[px] + 1) // 2 * 64) and np.array_equal(plans[px, 1], spp[px])
    assert np.array_equal(plans[sm, 0], total[sm]) and np.array_equal(plans[sm, 1], (spp[sm] + 1) // 2)
    assert ((patches[px] % 2) == 1).any() and ((spp[sm] % 2) == 1).any()  # unequal halves of both kinds


def test_two_full_of_unsplit_frames(lib):
    """Beside a split: two streams only for a remainder of at least a full batch less one sample of its pixels."""
    def two_full(patches, spp, max_paths):
        r = np.array([(PF_ANALYTIC, 1, patches, spp, 0, 1, max_paths, -1, 256, 8, 1, 0, 22, 1)], np.int64)
        return _plans(lib, r)[0]
    assert list(two_full(4, 4, 768)[[0, 1, 7]]) == [256, 3, 0]  # 768 + 256 paths: nothing to overlap
    assert list(two_full(4, 5, 768)[[0, 1, 7]]) == [256, 3, 1]  # 768 + 512: one sample less
    assert list(two_full(4, 6, 768)[[0, 1, 7]]) == [256, 3, 1]


@pytest.mark.parametrize("tile_p", [0, 1, 2, 3, 8])
def test_pixel_of_is_a_bijection_onto_the_patch_grid(lib, tile_p):
    for pxn, pyn, part in itertools.product(range(1, 10), range(1, 10), (0, 3)):
        ncols, H = pxn * 8 - (8 - part if part else 0), pyn * 8 - (8 - part if part else 0)
        for x_offset, x_delt, col_block in ((0, 1, 1), (1, 3, 1), (2, 3, 4)):
            # the image: wide enough for every owned column, or one column short of the last owned one
            full = ((ncols - 1) // col_block * x_delt + x_offset) * col_block + (ncols - 1) % col_block + 1 \
                if col_block > 1 else x_offset + (ncols - 1) * x_delt + 1
            for W in (full, full - 1):
                n = pxn * pyn * 64
                out = np.empty((n, 4), np.int32)
                lib.pixels(W, H, ncols, x_offset, x_delt, col_block, tile_p, out.ctypes.data)
                c, py, px, valid = out.T
                cell = py.astype(np.int64) * (pxn * 8) + c
                assert (c >= 0).all() and (c < pxn * 8).all() and (py >= 0).all() and (py < pyn * 8).all()
                assert np.array_equal(np.sort(cell), np.arange(n)), (tile_p, pxn, pyn)
                want_px = np.where(col_block > 1, ((c // col_block) * x_delt + x_offset) * col_block + c % col_block,
                                   x_offset + c * x_delt)
                inside = (c < ncols) & (py < H)
                assert np.array_equal(valid == 1, inside & (want_px < W)), (tile_p, pxn, pyn, W)
                assert np.array_equal(px[valid == 1], want_px[valid == 1])
                # a patch's 64 indices are its 8 x 8 pixels in raster order
                assert np.array_equal(c % 8, np.tile(np.arange(64) % 8, pxn * pyn))
                assert np.array_equal(py % 8, np.tile(np.arange(64) // 8, pxn * pyn))
                if tile_p == 0:
                    assert np.array_equal((py // 8) * pxn + c // 8, np.repeat(np.arange(pxn * pyn), 64))  # raster patches


# ---- the smallest and the odd frames (tests/test_gpu_frames.py renders them) ------------------------------------
def _plan_of(lib, profile, patches, spp, max_paths=2**25, split_min=22, persist=0):
    r = np.array([(profile, 1, patches, spp, 0, 1, max_paths, -1, 256, 8, persist, 1, split_min, 1)], np.int64)
    npix, nsb, pixel_major, tile_p, per, split_pixels, split, two, rows, cols = (int(x) for x in _plans(lib, r)[0])
    return dict(npix=npix, nsb=nsb, pixel_major=pixel_major, split=split, two_full=two, rows=rows, cols=cols)


def test_plans_of_one_patch_and_odd_frames(lib):
    """1 x 1 and 1 x 7 (one patch of 64 pixels, 1 or 7 of them in the image), 37 x 23 (15 patches) and 9 x 65 (18):
    one batch of every patch and sample by default; under JSRT_SPLIT_MIN=8 a one-patch frame of 3 samples (192 paths)
    stays whole while 15 and 18 patches split -- 8 + 7 and 9 + 9 patches pixel-major, 2 + 1 samples sample-major."""
    for profile, patches, spp in itertools.product(PROFILES, (1, 15, 18), (1, 2, 3)):
        p = _plan_of(lib, profile, patches, spp)
        assert (p["npix"], p["nsb"], p["rows"], p["cols"], p["split"]) == (patches * 64, spp, 1, 1, 0), (profile, patches, spp)
        assert p["pixel_major"] == (profile != PF_ANALYTIC)
    for profile, spp in itertools.product(PROFILES, (1, 2, 3)):
        p = _plan_of(lib, profile, 1, spp, split_min=8)
        assert (p["npix"], p["nsb"], p["rows"], p["cols"], p["split"]) == (64, spp, 1, 1, 0), (profile, spp)
    for patches, first in ((15, 8), (18, 9)):
        for spp in (2, 3):
            p = _plan_of(lib, PF_SDF, patches, spp, split_min=8)  # pixel-major: pixel halves
            assert (p["npix"], p["nsb"], p["rows"], p["cols"], p["split"], p["two_full"]) == (first * 64, spp, 1, 2, 1, 1)
            p = _plan_of(lib, PF_ANALYTIC, patches, spp, split_min=8)  # sample-major: sample halves
            assert (p["npix"], p["nsb"], p["rows"], p["cols"], p["split"], p["two_full"]) == (patches * 64, (spp + 1) // 2, 2, 1, 1, 1)
        for profile in PROFILES:  # one sample (SimpleRenderer), or persistent casts: never split
            assert _plan_of(lib, profile, patches, 1, split_min=8)["split"] == 0
        assert _plan_of(lib, PF_SDF, patches, 3, split_min=8, persist=1)["split"] == 0
    # the 20 x 12 ladder frame (6 patches, 2 samples) at max_paths 128: six batches in either path order
    p = _plan_of(lib, PF_ANALYTIC, 6, 2, max_paths=128)
    assert (p["npix"], p["nsb"], p["rows"], p["cols"]) == (128, 1, 2, 3)
    p = _plan_of(lib, PF_SDF, 6, 2, max_paths=128)
    assert (p["npix"], p["nsb"], p["rows"], p["cols"]) == (64, 2, 1, 6)
    # a batch is never smaller than one patch, however small max_paths
    p = _plan_of(lib, PF_ANALYTIC, 1, 3, max_paths=1)
    assert (p["npix"], p["nsb"], p["rows"], p["cols"]) == (64, 1, 3, 1)


def _pixels(lib, W, H, ncols, x_offset, x_delt, col_block, tile_p):
    n = ((ncols + 7) // 8) * ((H + 7) // 8) * 64
    out = np.empty((n, 4), np.int32)
    lib.pixels(W, H, ncols, x_offset, x_delt, col_block, tile_p, out.ctypes.data)
    return out


@pytest.mark.parametrize("tile_p", [0, 8])
def test_pixel_of_on_frames_below_a_patch(lib, tile_p):
    """The valid indices of a frame are its pixels, each once: 1 x 1 (index 0 of 64), 1 x 7 (a column: indices 0, 8,
    ... 48), 13 x 1 (a row over two patches), 37 x 23 and 9 x 65 (partial last patch row and column), one worker's
    columns (x_offset 2, x_delt 5 of 37: 7 columns), a column per worker (x_delt = W), a block-cyclic rank whose last
    block is partial (W = 37, col_block 8, rank 1 of 3: 8 + 5 columns) and no owned column at all."""
    def image_pixels(W, H, ncols, x_offset, x_delt, col_block=1):
        out = _pixels(lib, W, H, ncols, x_offset, x_delt, col_block, tile_p)
        v = out[out[:, 3] == 1]
        assert len(out) == ((ncols + 7) // 8) * ((H + 7) // 8) * 64
        return out, sorted((int(px), int(py)) for _, py, px, _ in v)
    out, px = image_pixels(1, 1, 1, 0, 1)
    assert px == [(0, 0)] and out[0, 3] == 1 and len(out) == 64
    out, px = image_pixels(1, 7, 1, 0, 1)
    assert px == [(0, y) for y in range(7)] and list(np.flatnonzero(out[:, 3])) == [8 * y for y in range(7)]
    out, px = image_pixels(13, 1, 13, 0, 1)
    assert px == [(x, 0) for x in range(13)] and len(out) == 128
    for W, H in ((37, 23), (9, 65), (7, 9), (13, 7)):
        out, px = image_pixels(W, H, W, 0, 1)
        assert px == [(x, y) for x in range(W) for y in range(H)], (W, H)
    out, px = image_pixels(37, 23, 7, 2, 5)
    assert px == [(x, y) for x in range(2, 37, 5) for y in range(23)] and len(out) == 3 * 64
    for k in (0, 12):
        out, px = image_pixels(13, 7, 1, k, 13)
        assert px == [(k, y) for y in range(7)]
    out, px = image_pixels(37, 23, 13, 1, 3, 8)
    assert px == [(x, y) for x in list(range(8, 16)) + list(range(32, 37)) for y in range(23)]
    assert len(_pixels(lib, 5, 23, 0, 1, 3, 8, tile_p)) == 0  # no owned column: no patch, no index
