#!/bin/sh
# TEST INFRASTRUCTURE: regenerate tests/golden/casts_edge/ (World.cast known answers at geometric edges)
# from the reference itself (needs the reference sources + node), one or more scenes per cast code path.
set -e
HERE=$(cd "$(dirname "$0")" && pwd)
OUT=$(cd "$HERE/../.." && pwd)/tests/golden/casts_edge
SCENES="cornell_box BoxBall spheres050 Aggregates AHollowTetrahedron AMultipleBVH bunny refraction SDF_BoxBall SDF_Menger"
rm -rf "$OUT"
node "$HERE/make_edge_cast_kats.js" "$OUT" $SCENES
gzip -9 -n -f "$OUT"/*.json
