"""Pins the C oracle to the reference at the recursion depths and frame shapes no other golden has.

tests/golden/frames/ (oracle/refharness/regen_frames.sh, spec_frames.json) holds frames the reference itself rendered
of the scenes of tests/golden/scenes/:
  * a depth ladder at 20 x 12, seed 3: maxRecursionDepth 1, 2, 3, 9, 12 and 16 (the library accepts 1 ... 16; every
    other golden is rendered at 4 ... 8), with one kind-0 and one kind-2 frame at depth 16;
  * shapes at each scene's own depth: 1 x 1, 13 x 1, 1 x 7, 7 x 9, 13 x 7, 9 x 65 and 37 x 23 (no multiple of the
    8 x 8 patch, a single row, a single column, primes), kinds 0, 1 and 2, and one worker's columns of 37 x 23.
As in test_oracle_golden.py the oracle must reproduce each bit for bit: the RGBA8 bytes, the f32 colour handed to
setColor (NaN equal to NaN) and the RNG draw / World.color call counts.

One more condition, no tolerance: the deep levels must be live.  A frame at depth D that equals the frame at depth
D - 1 says nothing about level D - 1, so for every ladder frame with D >= 2 the oracle's f32 frame at D must differ
from its frame at D - 1 in at least one pixel.  (The RGBA8 frames of cornell_box_path at 12 and 16 are identical at
this size: the f32 comparison is the one that counts.)  The ladder stops SDF_Menger at 9: above depth 12 its frames
no longer change, as Aggregates' above 6."""
import numpy as np
import pytest

from oracle import pyoracle

SUB = "frames"
RENDERS = pyoracle.golden_index(SUB)
LADDER = sorted(t for t, r in RENDERS.items() if (r["width"], r["height"]) == (20, 12))
SHAPES = sorted(set(RENDERS) - set(LADDER))

# what the ladder and the shapes must hold: a regenerated tree that lost a case fails here, not silently
LADDER_DEPTHS = {("cornell_box_path", 1): {1, 2, 3, 9, 12, 16}, ("refraction_path", 1): {1, 9, 16},
                 ("bunny", 1): {1, 2, 9, 16}, ("diamond", 1): {12, 16}, ("refraction", 1): {16},
                 ("SDF_Menger", 1): {1, 9}, ("cornell_box_path", 2): {16}, ("refraction", 0): {16}}
SHAPE_CASES = {("cornell_box_path", 37, 23, 1, 2, 0, 1), ("cornell_box_path", 1, 1, 1, 3, 0, 1),
               ("cornell_box_path", 13, 1, 0, 1, 0, 1), ("cornell_box_path", 1, 7, 2, 3, 0, 1),
               ("cornell_box_path", 9, 65, 1, 1, 0, 1), ("cornell_box_path", 37, 23, 1, 2, 2, 5),
               ("bunny", 37, 23, 0, 1, 0, 1), ("bunny", 7, 9, 2, 3, 0, 1), ("SDF_Menger", 13, 7, 1, 2, 0, 1),
               ("Aggregates", 7, 9, 1, 2, 0, 1)}


def _nan_equal_bits(a, b):
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


_frames = {}


def _oracle_frame(oracle, r, depth=None):
    """The oracle's frame of golden entry r (at another depth, for the liveness condition): computed once."""
    key = (r["scene"], r["width"], r["height"], r["spp"], depth or r["depth"], r["kind"], r["seed"], r["x_offset"], r["x_delt"])
    if key not in _frames:
        colors, rgba, st = oracle.render(oracle.golden_scene(key[0]), *key[1:])
        colors.setflags(write=False)
        rgba.setflags(write=False)
        _frames[key] = (colors, rgba, st)
    return _frames[key]


def test_frames_index_holds_the_cases():
    ladder = {}
    for t in LADDER:
        r = RENDERS[t]
        assert (r["seed"], r["x_offset"], r["x_delt"]) == (3, 0, 1) and r["spp"] == (1, 2, 3)[r["kind"]], t
        ladder.setdefault((r["scene"], r["kind"]), set()).add(r["depth"])
    assert ladder == LADDER_DEPTHS
    shapes = set()
    for t in SHAPES:
        r = RENDERS[t]
        assert r["seed"] == 3 and r["depth"] == pyoracle.scene_header(pyoracle.golden_scene(r["scene"]))["max_depth"], t
        shapes.add((r["scene"], r["width"], r["height"], r["kind"], r["spp"], r["x_offset"], r["x_delt"]))
    assert shapes == SHAPE_CASES and len(SHAPES) == len(SHAPE_CASES)


@pytest.mark.parametrize("tag", sorted(RENDERS))
def test_oracle_matches_reference(oracle, tag):
    r = RENDERS[tag]
    colors, rgba, st = _oracle_frame(oracle, r)
    gcol, grgba = oracle.golden_image(tag, r["width"], r["height"], sub=SUB)
    assert np.array_equal(rgba, grgba), f"{tag}: {int((rgba != grgba).any(-1).sum())} RGBA8 pixels differ"
    assert _nan_equal_bits(colors, gcol).all(), f"{tag}: f32 colours not bit-exact"
    assert st["draws"] == r["draws"]
    assert st["color_calls"] == r["color_calls"]


@pytest.mark.parametrize("tag", [t for t in LADDER if RENDERS[t]["depth"] >= 2])
def test_deepest_level_is_live(oracle, tag):
    """The frame at depth D differs from the frame at depth D - 1 (f32, NaN equal to NaN) in at least one pixel, so
    level D - 1 of the recursion contributes to the golden; and the golden is that frame (test_oracle_matches_reference)."""
    r = RENDERS[tag]
    deep, _, sd = _oracle_frame(oracle, r)
    shallow, _, ss = _oracle_frame(oracle, r, r["depth"] - 1)
    changed = int((~_nan_equal_bits(deep, shallow)).any(-1).sum())
    print(f"{tag}: {changed} of {r['width'] * r['height']} pixels change from depth {r['depth'] - 1} to {r['depth']}")
    assert changed >= 1, f"{tag}: level {r['depth'] - 1} changes no pixel"
    assert sd["color_calls"] > ss["color_calls"]  # ... and World.color was called at the new level


def test_partition_columns_match_the_full_frame(oracle):
    """renderers.js:88: worker 2 of 5 of the 37 x 23 frame writes its columns 2, 7, ... 32 as the full frame has them
    and leaves every other column zero (37 = 7 x 5 + 2: workers 0 and 1 own eight columns, this one seven)."""
    full = "cornell_box_path_incremental_37x23_s2_d8_seed3"
    gcol, grgba = oracle.golden_image(full, 37, 23, sub=SUB)
    pcol, prgba = oracle.golden_image(full + "_part2of5", 37, 23, sub=SUB)
    cols = list(range(2, 37, 5))
    assert len(cols) == 7
    assert np.array_equal(prgba[:, cols], grgba[:, cols]) and _nan_equal_bits(pcol[:, cols], gcol[:, cols]).all()
    assert not np.delete(prgba, cols, axis=1).any() and np.isnan(np.delete(pcol, cols, axis=1)).all()
