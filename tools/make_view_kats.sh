#!/bin/sh
# TEST INFRASTRUCTURE: regenerate tests/golden/views/ (frames of one scene from 5 cameras) from the
# reference itself (needs the reference checkout load_reference.js finds, and node).  One scene per code path:
# cornell_box_path the hybrid chain (Incremental, 3 spp), BoxBall_path the plain chain, Aggregates the tree (Simple),
# SDF_Menger the persistent march, bunny the BVH (RandomMultisampling, 2 spp), BoxBall_DOF the depth-of-field camera.
# The scenes are those of tests/golden/scenes/.  Touches nothing outside tests/golden/views.
set -e
HERE=$(cd "$(dirname "$0")" && pwd)
ROOT=$(cd "$HERE/.." && pwd)
OUT=$ROOT/tests/golden/views
rm -rf "$OUT"
node "$HERE/make_view_kats.js" "$OUT" "$ROOT/tests/golden/scenes" cornell_box_path:1:3 BoxBall_path:1:2 Aggregates:0:1 \
    SDF_Menger:1:1 bunny:2:2 BoxBall_DOF:1:2
