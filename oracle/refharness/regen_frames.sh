#!/bin/sh
# TEST INFRASTRUCTURE: regenerate tests/golden/frames/ -- frames of the reference scenes at the recursion depths and
# frame shapes no other golden has, every known answer computed by the reference itself (needs the reference + node):
#   images/<tag>.{rgba,f32}  index.json   make_goldens.js, spec_frames.json
#     depth ladder (20 x 12, seed 3): maxRecursionDepth 1, 2, 3, 9, 12, 16, where the deep levels still change pixels
#     shapes (each scene's own depth): 1 x 1, 13 x 1, 1 x 7, 7 x 9, 13 x 7, 9 x 65, 37 x 23, one x_offset 2 / x_delt 5
# The scenes are those of tests/golden/scenes/ (pyoracle.golden_scene(name)): the copy make_goldens.js writes is
# deleted.  Touches nothing outside tests/golden/frames.
set -e
HERE=$(cd "$(dirname "$0")" && pwd)
OUT=$(cd "$HERE/../.." && pwd)/tests/golden/frames
rm -rf "$OUT"
mkdir -p "$OUT"
node "$HERE/make_goldens.js" "$HERE/spec_frames.json" "$OUT"
rm -rf "$OUT/scenes"
# the wall time of a render is no known answer: without it the tree is reproduced byte for byte
node -e 'const fs = require("fs"), f = process.argv[1], d = JSON.parse(fs.readFileSync(f, "utf8"));
for (const r of Object.values(d.renders)) delete r.ms;
fs.writeFileSync(f, JSON.stringify(d, null, 1));' "$OUT/index.json"
