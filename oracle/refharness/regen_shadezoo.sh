#!/bin/sh
# TEST INFRASTRUCTURE: regenerate tests/golden/shadezoo/ -- the shading zoo (shade_zoo_scenes.js: this project's own
# scenes, built from the materials and lights no reference scene uses) with every known answer computed by the
# reference itself (needs the reference + node):
#   scenes/<name>.jsrt.gz  images/<tag>.{rgba,f32}  index.json   make_goldens.js, spec_shadezoo.json (28 x 20 renders)
#   casts/<name>.json.gz     World.cast: the 28 x 20 primary rays, 256 random rays, 256 shadow segments
#   material/<name>.json.gz  material_data over those rays; SDF.distance per SDF primitive
#   json/<name>.json.gz      the Serializer JSON of the scene
#   casts_light/<name>.json.gz  World.cast of segments from hit points to the lights' sample points, in groups of 64
#                            sharing an origin (make_light_cast_kats.js): what the shadow grid's root masks hold for
# Touches nothing outside tests/golden/shadezoo.
set -e
HERE=$(cd "$(dirname "$0")" && pwd)
OUT=$(cd "$HERE/../.." && pwd)/tests/golden/shadezoo
SCENES="shz_solid_transparent shz_phong_children shz_fresnel_edges shz_path_scatter shz_light_uv shz_light_mix shz_profiles_sdf shz_profiles_mesh shz_profiles_all"
rm -rf "$OUT"
mkdir -p "$OUT/json"
node "$HERE/make_goldens.js" "$HERE/spec_shadezoo.json" "$OUT"
gzip -9 -n -f "$OUT"/scenes/*.jsrt
node "$HERE/make_cast_kats.js" --primary=28x20 --random=256 --shadow=256 "$OUT/casts" $SCENES
gzip -9 -n -f "$OUT"/casts/*.json
node "$HERE/make_material_kats.js" "$OUT/casts" "$OUT/material" $SCENES
gzip -9 -n -f "$OUT"/material/*.json
node "$HERE/make_json_fixtures.js" "$OUT/json" $SCENES
gzip -9 -n -f "$OUT"/json/*.json
node "$HERE/make_light_cast_kats.js" "$OUT/casts_light" shz_solid_transparent shz_light_uv shz_light_mix shz_profiles_all
gzip -9 -n -f "$OUT"/casts_light/*.json
# the wall time of a render is no known answer: without it the tree is reproduced byte for byte
node -e 'const fs = require("fs"), f = process.argv[1], d = JSON.parse(fs.readFileSync(f, "utf8"));
for (const r of Object.values(d.renders)) delete r.ms;
fs.writeFileSync(f, JSON.stringify(d, null, 1));' "$OUT/index.json"
