#!/bin/sh
# TEST INFRASTRUCTURE: regenerate tests/golden/casts_light/ (World.cast known answers of shadow segments from
# hit points to light sample points) from the reference itself (needs the reference sources + node).
set -e
HERE=$(cd "$(dirname "$0")" && pwd)
OUT=$(cd "$HERE/../.." && pwd)/tests/golden/casts_light
SCENES="cornell_box BoxBall spheres050 Aggregates AHollowTetrahedron AMultipleBVH bunny refraction SDF_BoxBall SDF_Menger"
rm -rf "$OUT"
node "$HERE/make_light_cast_kats.js" "$OUT" $SCENES
gzip -9 -n -f "$OUT"/*.json
