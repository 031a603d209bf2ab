#!/bin/sh
# TEST INFRASTRUCTURE: regenerate tests/golden/posuv/ (the five PositionalUVMaterial thumbnail scenes, their reference
# renders and per-hit UV answers) from the reference itself (needs the reference checkout load_reference.js finds,
# and node).
set -e
HERE=$(cd "$(dirname "$0")" && pwd)
ROOT=$(cd "$HERE/.." && pwd)
OUT=$ROOT/tests/golden/posuv
MTL=$ROOT/tests/golden/mtlmap
rm -rf "$OUT" "$MTL"
node "$HERE/make_posuv_fixtures.js" "$OUT"
gzip -9 -n -f "$OUT"/*.jsrt "$OUT"/*.f32 "$OUT"/*.rgba "$OUT"/*.json
gunzip "$OUT"/scenes.json.gz
gzip -9 -n -f "$MTL"/*.jsrt "$MTL"/*.f32 "$MTL"/*.rgba "$MTL"/*.rgba8
