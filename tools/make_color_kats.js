"use strict";
/*
 * TEST INFRASTRUCTURE ONLY.  Known answers for World.color of single rays, computed by the reference itself
 * (vm-loaded by oracle/refharness/load_reference.js) under the keyed Math.random (oracle/refharness/keyed_rng.js):
 * the per-ray yardstick of the whole shade / shadow / reduce chain (include/jsrt_color.h, DESIGN.md §2.8).
 *
 * For each scene: the first 64 "primary" and the first 128 "random" rays of its cast known answers
 * (<casts dir>/<scene>.json.gz, same scene blob), ray i keyed as pixel i, samples 0 and 1, each through the
 * reference's own world.color(ray, depth) for depth 1 and the scene's maxRecursionDepth.  The root call is the
 * first child of the pre-root frame, as a renderer's is.  A scene whose first rays fall short of the checks below
 * (cornell_box_path: the first primary rays see the unlit ceiling) takes the same number of rays evenly spaced over
 * the same sets instead.
 *
 *   node tools/make_color_kats.js <outdir> <casts dir>:<scene>...
 * writes <outdir>/<scene>.json: {scene, blob_sha256, seed, n, samples, rays (base64 f32 n x 6), hit (base64 u8 n),
 *   depths, rgb (base64 f32, depth x n x samples x 3)}
 *
 * Asserted per scene and depth (tests/test_gpu_color.py asserts them again): no ray makes the reference throw,
 * every value is finite, at least half the rays hit something, at least a quarter of the hits have a colour no
 * other hit has, and for cornell_box_path at least a quarter of the hits differ between the two samples.
 */
const fs = require("fs");
const path = require("path");
const zlib = require("zlib");
const crypto = require("crypto");
const { loadScene, refClass } = require("../oracle/refharness/load_reference");
const { installKeyedRng } = require("../oracle/refharness/keyed_rng");
const { SceneBlobWriter } = require("../jsraytracer_amd/js/scene_blob");

const SEED = 1, SAMPLES = 2, TAKE = { primary: 64, random: 128 };
const b64 = (typed) => Buffer.from(typed.buffer, typed.byteOffset, typed.byteLength).toString("base64");
const unb64 = (str, T) => { const b = Buffer.from(str, "base64"); return new T(b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength)); };

// the colours of one choice of rays (spaced: evenly over each set, not its first ones); throws where a check fails
function evaluate(name, test, kat, sha, spaced) {
    const world = test.renderer.world;
    const Vec = refClass("Vec"), Ray = refClass("Ray"), World = refClass("World");
    const rr = [];
    for (const set of kat.sets) {
        if (!(set.name in TAKE)) continue;
        const R = unb64(set.rays, Float32Array);
        const take = Math.min(set.n, TAKE[set.name]), step = spaced ? Math.floor(set.n / take) : 1;
        for (let k = 0; k < take * step; k += step) rr.push(Array.from(R.subarray(6 * k, 6 * k + 6)));
    }
    const n = rr.length;
    const rays = rr.map(r => new Ray(Vec.of(r[0], r[1], r[2], 1), Vec.of(r[3], r[4], r[5], 0)));
    const RR = Float32Array.from([].concat(...rr));
    const HIT = Uint8Array.from(rays.map(ray => (world.cast(ray).object == null ? 0 : 1)));
    const hits = HIT.reduce((a, b) => a + b, 0);
    const depths = [1, test.renderer.maxRecursionDepth];
    const RGB = new Float32Array(depths.length * n * SAMPLES * 3);
    const random = Math.random;
    const ctl = installKeyedRng(SEED);
    try {
        depths.forEach((depth, d) => rays.forEach((ray, i) => {
            for (let s = 0; s < SAMPLES; ++s) {
                ctl.startSequence([[i, s]][Symbol.iterator]());
                const c = world.color(ray, depth);  // (a throw ends the run: no ray may make the reference throw)
                for (let j = 0; j < 3; ++j) RGB[((d * n + i) * SAMPLES + s) * 3 + j] = c[j];
            }
        }));
    } finally {
        Math.random = random;
        World.prototype.color = World.prototype.__jsrt_orig_color;
    }
    if (!RGB.every(Number.isFinite)) throw new Error(`${name}: a colour is not finite`);
    if (2 * hits < n) throw new Error(`${name}: only ${hits} of ${n} rays hit`);
    const info = [];
    depths.forEach((depth, d) => {
        const of = (i) => Array.from(RGB.subarray((d * n + i) * SAMPLES * 3, (d * n + i + 1) * SAMPLES * 3));
        const count = new Map();
        let differ = 0;
        for (let i = 0; i < n; ++i) {
            if (!HIT[i]) continue;
            const c = of(i), k = c.join(",");
            count.set(k, (count.get(k) || 0) + 1);
            if (c[0] !== c[3] || c[1] !== c[4] || c[2] !== c[5]) ++differ;
        }
        let unique = 0;
        for (const v of count.values()) if (v === 1) ++unique;
        if (4 * unique < hits) throw new Error(`${name} depth ${depth}: only ${unique} of ${hits} hits have a colour of their own`);
        if (name === "cornell_box_path" && 4 * differ < hits)
            throw new Error(`${name} depth ${depth}: only ${differ} of ${hits} hits differ between the samples`);
        info.push(`depth ${depth}: ${unique} distinct, ${differ} differ between samples`);
    });
    console.log(`${name}: ${n} rays${spaced ? " (evenly spaced)" : ""}, ${hits} hits; ${info.join("; ")}`);
    return { scene: name, blob_sha256: sha, seed: SEED, n, samples: SAMPLES, rays: b64(RR), hit: b64(HIT), depths, rgb: b64(RGB) };
}

async function main() {
    const outdir = path.resolve(process.argv[2]);
    fs.mkdirSync(outdir, { recursive: true });
    for (const arg of process.argv.slice(3)) {
        const [castsDir, name] = arg.split(":");
        const test = await loadScene(name);
        const blob = new SceneBlobWriter().build(test);
        const kat = JSON.parse(zlib.gunzipSync(fs.readFileSync(path.join(path.resolve(castsDir), name + ".json.gz"))));
        const sha = crypto.createHash("sha256").update(blob).digest("hex");
        if (sha !== kat.blob_sha256) throw new Error(`${name}: scene blob differs from the cast KATs' blob`);
        let out;
        try {
            out = evaluate(name, test, kat, sha, false);
        } catch (e) {
            console.log(`${e.message}: taking evenly spaced rays`);
            out = evaluate(name, test, kat, sha, true);
        }
        fs.writeFileSync(path.join(outdir, name + ".json"), JSON.stringify(out));
    }
}
main().catch(e => { console.error(e); process.exit(1); });
