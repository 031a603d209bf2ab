#!/bin/sh
# TEST INFRASTRUCTURE: regenerate tests/golden/sdfzoo/ -- the SDF zoo (zoo_scenes.js: this project's own scenes,
# whose SDF roots match no recognised program form) with every known answer computed by the reference itself
# (needs the reference + node):
#   scenes/<name>.jsrt.gz  images/<tag>.{rgba,f32}  index.json   make_goldens.js, spec_zoo.json (28 x 20 renders)
#   casts/<name>.json.gz     World.cast: the 28 x 20 primary rays, 256 random rays, 256 shadow segments
#   material/<name>.json.gz  material_data over those rays; SDF.distance per SDF primitive
#   json/<name>.json.gz      the Serializer JSON of the scene
# Touches nothing outside tests/golden/sdfzoo.
set -e
HERE=$(cd "$(dirname "$0")" && pwd)
OUT=$(cd "$HERE/../.." && pwd)/tests/golden/sdfzoo
SCENES="zoo_round_nary zoo_union_wide zoo_nested_tx zoo_loops zoo_smooth_chain zoo_mixed"
rm -rf "$OUT"
mkdir -p "$OUT/json"
node "$HERE/make_goldens.js" "$HERE/spec_zoo.json" "$OUT"
gzip -9 -n -f "$OUT"/scenes/*.jsrt
node "$HERE/make_cast_kats.js" --primary=28x20 --random=256 --shadow=256 "$OUT/casts" $SCENES
gzip -9 -n -f "$OUT"/casts/*.json
node "$HERE/make_material_kats.js" "$OUT/casts" "$OUT/material" $SCENES
gzip -9 -n -f "$OUT"/material/*.json
node "$HERE/make_json_fixtures.js" "$OUT/json" $SCENES
gzip -9 -n -f "$OUT"/json/*.json
