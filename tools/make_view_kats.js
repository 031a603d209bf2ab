"use strict";
/*
 * TEST INFRASTRUCTURE ONLY.  Known answers for frames of one scene seen from several cameras, rendered by the
 * reference itself (vm-loaded by oracle/refharness/load_reference.js) under the keyed Math.random
 * (oracle/refharness/keyed_rng.js): the yardstick of include/jsrt_views.h (DESIGN.md §2.9).
 *
 * For each scene the reference scene is loaded once; then, for each of 5 views, the live camera is moved with the
 * reference's own Camera.setTransform (cameras.js:6-9) -- views 2 and 4 also call changeFOV (cameras.js:25-28), and
 * on a DepthOfFieldPerspectiveCamera views 1 and 3 also change focus_distance / sensor_size -- and the frame is
 * rendered at 20 x 12 with the scene's own maxRecursionDepth.  View 0 is the scene's own camera, untouched.
 *
 *   node tools/make_view_kats.js <outdir> <scenes dir> <scene>:<kind>:<spp>...
 * writes <outdir>/<scene>/cameras.json: {scene, blob_sha256, kind, spp, depth, seed, width, height, views: [{kind,
 *   transform (16 f64, Mat rows), tan_fov, aspect, focus_distance, sensor_size}]} -- the numbers read back from the
 *   live camera object after the calls above -- and per view <outdir>/<scene>/view<k>.rgba (the ImageData bytes) and
 *   view<k>.f32 (the colour handed to PixelBuffer.setColor per pixel, f32 x 4, NaN-padded).
 *
 * Refused (nothing is written for the scene): a scene whose exported blob is not the committed
 * <scenes dir>/<scene>.jsrt.gz, and a scene two of whose views have identical RGBA8 -- a camera that is ignored
 * must fail the tests.
 */
const fs = require("fs");
const path = require("path");
const zlib = require("zlib");
const crypto = require("crypto");
const { loadScene, refClass } = require("../oracle/refharness/load_reference");
const { installKeyedRng, sampleOrder } = require("../oracle/refharness/keyed_rng");
const { exportScene } = require("../jsraytracer_amd/js/scene_blob");

const SEED = 3, W = 20, H = 12, VIEWS = 5;

function makeRenderer(test, kind, spp) {
    const R = test.renderer, d = R.maxRecursionDepth;
    if (kind === 0) return new (refClass("SimpleRenderer"))(R.world, R.camera, d);
    if (kind === 1) return new (refClass("IncrementalMultisamplingRenderer"))(R.world, R.camera, spp, d);
    return new (refClass("RandomMultisamplingRenderer"))(R.world, R.camera, spp, d);
}

// the camera of view v > 0: the scene's own transform T0, turned and shifted in its own frame
function moveCamera(C, v, T0, fov0, focus0, sensor0) {
    const Mat4 = refClass("Mat4"), Vec = refClass("Vec");
    const turn = [null, [0.12, Vec.of(0, 1, 0)], [-0.1, Vec.of(1, 0, 0)], [0.2, Vec.of(0, 1, 1)], [-0.15, Vec.of(1, 1, 0)]][v];
    const shift = [null, [0.3, 0.1, 0], [-0.2, 0.25, 0.4], [0.1, -0.2, -0.3], [-0.35, 0.05, 0.2]][v];
    C.setTransform(T0.times(Mat4.translation(shift)).times(Mat4.rotation(turn[0], turn[1])));
    if (v === 2) C.changeFOV(fov0 * 0.8);
    if (v === 4) C.changeFOV(fov0 * 1.15);
    if (focus0 !== undefined && v === 1) C.focus_distance = focus0 * 0.8;
    if (focus0 !== undefined && v === 3) { C.focus_distance = focus0 * 1.3; C.sensor_size = sensor0 * 2; }
}

function readCamera(C) {
    const dof = C.constructor.name === "DepthOfFieldPerspectiveCamera";
    const t = [];
    for (let r = 0; r < 4; ++r) for (let c = 0; c < 4; ++c) t.push(C.transform[r][c]);
    return { kind: dof ? 1 : 0, transform: t, tan_fov: C.tan_fov, aspect: C.aspect,
             focus_distance: dof ? C.focus_distance : 0, sensor_size: dof ? C.sensor_size : 0 };
}

async function main() {
    const outroot = path.resolve(process.argv[2]), scenes = path.resolve(process.argv[3]);
    const PixelBuffer = refClass("PixelBuffer");
    for (const arg of process.argv.slice(4)) {
        const [name, kindS, sppS] = arg.split(":");
        const kind = Number(kindS), spp = kind === 0 ? 1 : Number(sppS);
        const test = await loadScene(name);
        const blob = exportScene(test);
        const committed = zlib.gunzipSync(fs.readFileSync(path.join(scenes, name + ".jsrt.gz")));
        if (Buffer.compare(Buffer.from(blob.buffer || blob, blob.byteOffset || 0, blob.length), committed) !== 0)
            throw new Error(`${name}: the exported scene blob differs from ${scenes}/${name}.jsrt.gz`);
        const C = test.renderer.camera;
        const T0 = C.transform, fov0 = C.FOV, focus0 = C.focus_distance, sensor0 = C.sensor_size;
        const renderer = makeRenderer(test, kind, spp);
        const views = [], images = [];
        for (let v = 0; v < VIEWS; ++v) {
            if (v > 0) moveCamera(C, v, T0, fov0, focus0, sensor0);
            const colors = new Float32Array(W * H * 4).fill(NaN);
            const pb = new PixelBuffer(W, H);
            const origSet = PixelBuffer.prototype.setColor;
            pb.setColor = function (x, y, color) {
                const i = y * W + x;
                for (let k = 0; k < 4; ++k) colors[4 * i + k] = k < color.length ? color[k] : NaN;
                return origSet.call(this, x, y, color);
            };
            const ctl = installKeyedRng(SEED);
            ctl.startSequence(sampleOrder(kind, W, H, spp, 0, 1));
            renderer.render(pb, 0, false, 0, 1);
            views.push(readCamera(C));
            images.push({ rgba: Buffer.from(pb.imgdata.data.buffer).subarray(0, W * H * 4), f32: Buffer.from(colors.buffer) });
        }
        for (let a = 0; a < VIEWS; ++a)
            for (let b = a + 1; b < VIEWS; ++b)
                if (Buffer.compare(images[a].rgba, images[b].rgba) === 0)
                    throw new Error(`${name}: views ${a} and ${b} have identical RGBA8`);
        for (const view of views)
            for (const x of view.transform.concat([view.tan_fov, view.aspect, view.focus_distance, view.sensor_size]))
                if (!Number.isFinite(x)) throw new Error(`${name}: a camera number is not finite`);
        const out = path.join(outroot, name);
        fs.mkdirSync(out, { recursive: true });
        images.forEach((im, v) => {
            fs.writeFileSync(path.join(out, `view${v}.rgba`), im.rgba);
            fs.writeFileSync(path.join(out, `view${v}.f32`), im.f32);
        });
        fs.writeFileSync(path.join(out, "cameras.json"), JSON.stringify({
            scene: name, blob_sha256: crypto.createHash("sha256").update(committed).digest("hex"), kind, spp,
            depth: test.renderer.maxRecursionDepth, seed: SEED, width: W, height: H, views }, null, 1));
        console.log(`${name}: ${VIEWS} views, kind ${kind}, ${spp} spp, depth ${test.renderer.maxRecursionDepth}`);
    }
}
main().catch(e => { console.error(e); process.exit(1); });
