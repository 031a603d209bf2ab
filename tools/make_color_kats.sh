#!/bin/sh
# TEST INFRASTRUCTURE: regenerate tests/golden/colors/ (World.color known answers per ray) from the
# reference itself (needs the reference checkout load_reference.js finds, and node), over the rays of the cast known
# answers.  cornell_box_path, refraction, BoxBall_DOF and the zoo scene take the hybrid chain schedule, BoxBall_path (no
# material with two children) the plain chain, the BVH, aggregate and SDF scenes the tree.  The shading zoo's scene is
# loaded as regen_shadezoo.sh loads it, over its own casts.
set -e
HERE=$(cd "$(dirname "$0")" && pwd)
ROOT=$(cd "$HERE/.." && pwd)
OUT=$ROOT/tests/golden/colors
C=$ROOT/tests/golden/casts
Z=$ROOT/tests/golden/shadezoo/casts
rm -rf "$OUT"
node "$HERE/make_color_kats.js" "$OUT" "$C:cornell_box_path" "$C:refraction" "$C:Aggregates" "$C:AMultipleBVH" \
    "$C:SDF_Combinations" "$C:SDF_Menger" "$C:BoxBall_DOF" "$C:BoxBall_path" "$Z:shz_solid_transparent"
gzip -9 -n -f "$OUT"/*.json
