#!/bin/sh
# TEST INFRASTRUCTURE: regenerate tests/golden/texture/ (TextureMaterialColor known answers and the four textured
# thumbnail scenes) from the reference itself (needs the reference checkout load_reference.js finds, and node).
set -e
HERE=$(cd "$(dirname "$0")" && pwd)
ROOT=$(cd "$HERE/.." && pwd)
OUT=$ROOT/tests/golden/texture
rm -rf "$OUT"
node "$HERE/make_texture_fixtures.js" "$OUT"
gzip -9 -n -f "$OUT"/*.jsrt "$OUT"/*.bin "$OUT"/*.f32 "$OUT"/*.rgba "$OUT"/kats.json
