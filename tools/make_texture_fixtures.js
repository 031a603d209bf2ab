"use strict";
/*
 * TEST INFRASTRUCTURE ONLY.  Generates tests/golden/texture/ by running the REFERENCE's own code (loaded at run
 * time by oracle/refharness/load_reference.js; nothing of it is copied): known answers of
 * TextureMaterialColor.color (src/materials.js:101-130) and four 32x24 textured scenes rendered by the reference's
 * renderers with the keyed RNG (oracle/refharness/keyed_rng.js), each stored as its exported blob
 * (jsraytracer_amd/js/scene_blob.js) plus the reference's image.  Images and scenes are built here, from the
 * reference's classes; the output is data only.
 *
 *   node tools/make_texture_fixtures.js <outdir>        (tools/make_texture_fixtures.sh)
 *
 * kats.jsrt   a blob whose MCOL section holds every known-answer colour chain (and their textures)
 * kats.bin    f32: the UV sets (n x 2 each), then per case its n x 3 results (r, g, b of the returned Vec)
 * kats.json   {uv_sets: [{size, n, offset}], cases: [{id, mcolor, kind, uv_set, n, offset, ...}]} (offsets in f32s)
 * <scene>.jsrt / .rgba / .f32 and scenes.json: as oracle/refharness/make_goldens.js writes them
 * mesh_untextured.jsrt  scene 3 with a solid colour where its texture is (same MCOL index): the input of the
 *                       jsrt_blob_set_texture route
 *
 * Per scene the generator asserts that the reference's render threw nothing, that every colour it set had three
 * components, that at least a quarter of the pixels' primary hits evaluate a texture and that at least a tenth of
 * those evaluations have a UV pair outside [0, 1]^2 -- or it fails.
 */
const fs = require("fs");
const path = require("path");
const { refClass } = require("../oracle/refharness/load_reference");
const { installKeyedRng, sampleOrder } = require("../oracle/refharness/keyed_rng");
const { SceneBlobWriter, exportScene } = require("../jsraytracer_amd/js/scene_blob");

const C = (n) => refClass(n);
const outdir = path.resolve(process.argv[2] || "tests/golden/texture");
fs.mkdirSync(outdir, { recursive: true });

// ---- deterministic helpers -------------------------------------------------------------------------------
function rng32(seed) {  // mulberry32
    let a = seed >>> 0;
    return () => {
        a = (a + 0x6D2B79F5) >>> 0;
        let t = a;
        t = Math.imul(t ^ (t >>> 15), t | 1);
        t ^= t + Math.imul(t ^ (t >>> 7), t | 61);
        return ((t ^ (t >>> 14)) >>> 0) / 4294967296;
    };
}
function image(w, h, seed) {  // an ImageData-like {width, height, data}: seeded bytes, 0 and 255 among them
    const r = rng32(seed), data = new Uint8ClampedArray(w * h * 4);
    for (let i = 0; i < data.length; ++i) data[i] = Math.floor(r() * 256);
    for (let i = 0; i < data.length; i += 5) data[i] = (i % 2) ? 255 : 0;
    return { width: w, height: h, data };
}
const f32buf = new Float32Array(1), u32buf = new Uint32Array(f32buf.buffer);
function f32(x) { f32buf[0] = x; return f32buf[0]; }
function ulp(x, d) {  // the f32 next to f32(x) in direction d (+1 / -1), through +-0
    f32buf[0] = x;
    if (f32buf[0] === 0) { u32buf[0] = d > 0 ? 1 : 0x80000001; return f32buf[0]; }
    u32buf[0] += (f32buf[0] > 0) === (d > 0) ? 1 : -1;
    return f32buf[0];
}

// ---- known answers ---------------------------------------------------------------------------------------
const SIZES = [[1, 1], [1, 4], [4, 1], [2, 2], [5, 3], [64, 64]];
function axisSpecials(n) {  // U (or V) values for a texture of n texels along the axis
    const base = [0, 1, -0, 0.5 / n, 1 - 0.5 / n];
    const idx = n <= 8 ? [...Array(n).keys()] : [0, 1, 2, n >> 1, n - 3, n - 2, n - 1];
    for (const i of idx) base.push((i + 0.5) / n, i / n, (i + 1) / n);  // texel centres and edges
    base.push(-0.25, 1.25, -1, 2, 0.5);  // the same structure one period away (wrap) / clamped away
    const out = [];
    for (const b of base) out.push(f32(b), ulp(b, 1), ulp(b, -1));
    out.push(1e30, -1e30, Infinity, -Infinity, NaN);
    return out;
}
function uvSet(w, h, seed) {
    const r = rng32(seed), uv = [];
    const U = axisSpecials(w), V = axisSpecials(h);
    const rnd = () => f32(-2 + 5 * r());
    for (const u of U) { uv.push([u, rnd()], [u, V[Math.floor(r() * V.length)]]); }
    for (const v of V) { uv.push([rnd(), v], [U[Math.floor(r() * U.length)], v]); }
    for (let i = 0; i < Math.max(U.length, V.length); ++i) uv.push([U[i % U.length], V[i % V.length]]);
    uv.push([NaN, 0.3], [0.3, NaN], [NaN, NaN], [Infinity, Infinity], [-Infinity, 0.5], [0.5, -Infinity]);
    for (let i = 0; i < 400; ++i) uv.push([rnd(), rnd()]);
    return uv;
}

function makeKats() {
    const Tex = C("TextureMaterialColor"), Scaled = C("ScaledMaterialColor"), Checker = C("CheckerboardMaterialColor");
    const Vec = C("Vec");
    const writer = new SceneBlobWriter();
    const floats = [], uvSets = [], cases = [];
    const sets = SIZES.map(([w, h], i) => {
        const uv = uvSet(w, h, 1000 + i);
        uvSets.push({ size: [w, h], n: uv.length, offset: floats.length });
        for (const [u, v] of uv) floats.push(u, v);
        return uv;
    });
    const run = (id, mc, set, extra) => {
        const uv = sets[set];
        const c = Object.assign({ id, mcolor: writer.mcIndex(mc), uv_set: set, n: uv.length, offset: floats.length }, extra);
        for (const [u, v] of uv) {
            const col = mc.color({ UV: Vec.of(u, v) });  // (Vec: the UV is f32, as every geometry's is)
            floats.push(col[0], col[1], col[2]);
        }
        cases.push(c);
    };
    const images = SIZES.map(([w, h], i) => image(w, h, 7 + i));
    const byKey = {};
    SIZES.forEach(([w, h], si) => {
        for (const mode of ["bilinear", "nearest"])
            for (const cu of [true, false])
                for (const cv of [true, false]) {
                    const t = new Tex(images[si], mode, cu, cv);
                    byKey[`${w}x${h}_${mode}_${+cu}${+cv}`] = t;
                    run(`tex_${w}x${h}_${mode}_u${+cu}_v${+cv}`, t, si, { kind: "texture", size: [w, h], mode, clampU: cu, clampV: cv });
                }
    });
    // chains over the same textures (ScaledMaterialColor, CheckerboardMaterialColor: materials.js:43-76)
    const t53 = byKey["5x3_bilinear_01"], t22 = byKey["2x2_nearest_00"], t64 = byKey["64x64_bilinear_11"];
    run("scaled_scalar_5x3", new Scaled(t53, 0.3), 4, { kind: "scaled_scalar", of: "tex_5x3_bilinear_u0_v1", scale: 0.3 });
    run("scaled_vec_64x64", new Scaled(t64, Vec.of(0.5, 0.75, 0.25)), 5,
        { kind: "scaled_vec", of: "tex_64x64_bilinear_u1_v1", scale: [0.5, 0.75, 0.25] });
    run("checker_5x3_2x2", new Checker(t53, new Scaled(t22, 0.5)), 4,
        { kind: "checker", a: "tex_5x3_bilinear_u0_v1", b: "tex_2x2_nearest_u0_v0", b_scale: 0.5 });
    // (the 2x2 texture on the 5x3 UV set, for the checkerboard's second colour)
    run("tex_2x2_nearest_u0_v0_on_5x3", t22, 4, { kind: "texture", size: [2, 2], mode: "nearest", clampU: false, clampV: false });

    // a minimal world around the colour records (the exporter writes every record it was asked to index)
    const world = new (C("World"))(
        [new (C("Primitive"))(new (C("Square"))(), new (C("PhongMaterial"))(Vec.of(1, 1, 1), 0.5, 0.5))],
        [new (C("SimplePointLight"))(Vec.of(0, 0, 3, 1), Vec.of(1, 1, 1), 10)]);
    const cam = new (C("PerspectiveCamera"))(Math.PI / 4, 1, C("Mat4").translation([0, 0, 3]));
    const blob = writer.build({ renderer: new (C("SimpleRenderer"))(world, cam, 1), width: 8, height: 8 });
    fs.writeFileSync(path.join(outdir, "kats.jsrt"), blob);
    fs.writeFileSync(path.join(outdir, "kats.bin"), Buffer.from(Float32Array.from(floats).buffer));
    fs.writeFileSync(path.join(outdir, "kats.json"), JSON.stringify({ uv_sets: uvSets, cases }, null, 1));
    console.log(`kats: ${cases.length} cases, ${floats.length * 4} B of f32, blob ${blob.length} B`);
}

// ---- scenes ----------------------------------------------------------------------------------------------
const W = 32, H = 24;
function scenes() {
    const Vec = C("Vec"), Mat4 = C("Mat4"), Prim = C("Primitive"), Tex = C("TextureMaterialColor");
    const Phong = C("PhongMaterial"), Fresnel = C("FresnelPhongMaterial"), Path = C("PhongPathTracingMaterial");
    const Scaled = C("ScaledMaterialColor"), Checker = C("CheckerboardMaterialColor"), Solid = C("SolidMaterialColor");
    const Point = C("SimplePointLight"), World = C("World"), Cam = C("PerspectiveCamera");
    const rotX = (a) => Mat4.rotation(a, Vec.of(1, 0, 0)), rotY = (a) => Mat4.rotation(a, Vec.of(0, 1, 0));
    const out = {};

    {   // 1: flat analytic scene, SimpleRenderer, depth 2 (the LDS-staged k_shade)
        const floorTex = new Tex(image(8, 8, 101), "bilinear", true, true);
        const ballDiff = new Tex(image(6, 4, 102), "nearest", false, false);
        const ballSpec = new Tex(image(3, 5, 103), "bilinear", false, true);
        const objects = [
            new Prim(new (C("Square"))(), new Phong(Vec.of(1, 1, 1), floorTex, floorTex, 0.25, 10, 0.25),
                     Mat4.translation([0, -1, -4]).times(rotX(-Math.PI / 2)).times(Mat4.scale(9))),
            new Prim(new (C("Sphere"))(), new Phong(Vec.of(1, 0.75, 0.5), 0.125, ballDiff, ballSpec, 20),
                     Mat4.translation([0.25, 0, -4])),
        ];
        const world = new World(objects, [new Point(Vec.of(3, 5, 0, 1), Vec.of(1, 1, 1), 150)], Vec.of(0.125, 0.125, 0.25));
        out.flat = { test: { renderer: new (C("SimpleRenderer"))(world, new Cam(Math.PI / 3, W / H, Mat4.translation([0, 0.5, 0]).times(rotX(-0.2))), 2), width: W, height: H },
                     kind: 0, spp: 1, depth: 2, seed: 5 };
    }
    {   // 2: a closed box, one wall with a textured diffusivity, one Square area light of 4 samples; Incremental, 4 spp,
        //    depth 3 (the hybrid chain, k_shadow_node, the HAND_DIFF plane)
        const wallTex = new Tex(image(7, 5, 201), "bilinear", false, true);
        const wall = (col, T) => new Prim(new (C("Square"))(), new Path(Vec.of(1, 1, 1), 0, col), T);
        const objects = [
            wall(wallTex, Mat4.translation([0, 5, -5]).times(Mat4.scale([10, 10, 1]))),                       // back, textured
            wall(0.5, Mat4.translation([0, 5, 16]).times(Mat4.scale([10, 10, 1]))),                           // behind the camera
            new Prim(new (C("Square"))(), new Path(Vec.of(1, 0.125, 0.125), 0, 0.5),
                     Mat4.translation([5, 5, 5]).times(Mat4.scale([1, 10, 22])).times(rotY(Math.PI / 2))),
            new Prim(new (C("Square"))(), new Path(Vec.of(0.125, 1, 0.125), 0, 0.5),
                     Mat4.translation([-5, 5, 5]).times(Mat4.scale([1, 10, 22])).times(rotY(-Math.PI / 2))),
            wall(0.5, Mat4.translation([0, 0, 5]).times(Mat4.scale([10, 1, 22])).times(rotX(Math.PI / 2))),     // floor
            wall(0.5, Mat4.translation([0, 10, 5]).times(Mat4.scale([10, 1, 22])).times(rotX(Math.PI / 2))),    // ceiling
            new Prim(new (C("Sphere"))(), new Path(Vec.of(1, 1, 1), 0, 0.125, 0.75, 10, 2), Mat4.translation([-2.5, 1.5, 0]).times(Mat4.scale(1.5))),
        ];
        const light = new (C("RandomSampleAreaLight"))(new (C("Square"))(),
            Mat4.translation([0, 9.5, 0]).times(rotX(-Math.PI / 2)).times(Mat4.scale([2, 2, 1])), Vec.of(1, 1, 1), 600, 4);
        const world = new World(objects, [light]);
        out.box = { test: { renderer: new (C("IncrementalMultisamplingRenderer"))(world, new Cam(Math.PI / 4, W / H, Mat4.translation([0, 5, 15])), 4, 3), width: W, height: H },
                    kind: 1, spp: 4, depth: 3, seed: 9 };
    }
    // 3: a BVHAggregate of 40 triangles with per-vertex UVs (some outside [0, 1]), FresnelPhong, lit from behind (the
    //    transmission side carries 1 - kr of the diffuse term, materials.js:349-352)
    const mesh = (diffLeaf) => {
        const mat = new Fresnel(Vec.of(1, 1, 1), 0.125, new Scaled(diffLeaf, Vec.of(0.5, 0.75, 1)), 0.25, 10, 1.5);
        const nx = 5, ny = 4, tris = [];
        const P = (i, j) => Vec.of(-2.5 + i, -2 + j, -6 + 0.25 * Math.sin(1.5 * i) * Math.cos(1.25 * j), 1);
        const UV = (i, j) => Vec.of(-0.5 + 2 * i / nx, 1.5 - 2 * j / ny);
        for (let i = 0; i < nx; ++i)
            for (let j = 0; j < ny; ++j) {
                const q = [[i, j], [i + 1, j], [i + 1, j + 1], [i, j + 1]];
                for (const t of [[0, 1, 2], [0, 2, 3]])
                    tris.push(new Prim(new (C("Triangle"))(t.map(k => P(...q[k])), { UV: t.map(k => UV(...q[k])) }), mat));
            }
        const world = new World([C("BVHAggregate").build(tris)], [new Point(Vec.of(2, 3, -11, 1), Vec.of(1, 1, 1), 120)], Vec.of(0.25, 0.125, 0.125));
        return { test: { renderer: new (C("SimpleRenderer"))(world, new Cam(Math.PI / 4, W / H, Mat4.translation([0, 0, 0.5])), 3), width: W, height: H },
                 kind: 0, spp: 1, depth: 3, seed: 3 };
    };
    const meshTex = new Tex(image(9, 6, 301), "bilinear", false, false);
    out.mesh = mesh(meshTex);
    out.mesh_untextured = Object.assign(mesh(new Solid(Vec.of(0.5, 0.5, 0.5))), { no_render: true });
    {   // 4: a Cylinder and a UnitBox with Checkerboard(texture, Scaled(texture2, 0.5)) in ambient; 5x3, wrap U, clamp V.
        //    AABB.materialData supplies no UV (geometry.js:222), so the reference throws on any shaded hit of the box:
        //    it stands outside every camera and bounce ray's reach, where it only casts its shadow on the cylinder.
        const chain = new Checker(new Tex(image(5, 3, 401), "bilinear", false, true), new Scaled(new Tex(image(4, 4, 402), "nearest", true, false), 0.5));
        const mat = new Phong(Vec.of(1, 1, 1), chain, 0.5, 0.25, 10);
        const objects = [
            new Prim(new (C("Cylinder"))(), mat, Mat4.translation([0, 0, -4]).times(rotX(Math.PI / 2 - 0.3)).times(Mat4.scale([1.5, 1.5, 2.25]))),
            new Prim(new (C("UnitBox"))(), mat, Mat4.translation([1.5, 1.75, 1.5]).times(Mat4.scale(1.25))),
        ];
        const world = new World(objects, [new Point(Vec.of(3, 3.5, 7, 1), Vec.of(1, 1, 1), 200)], Vec.of(0.125, 0.25, 0.125));
        out.cylinder = { test: { renderer: new (C("SimpleRenderer"))(world, new Cam(Math.PI / 4, W / H, Mat4.translation([0, 0, 1])), 2), width: W, height: H },
                         kind: 0, spp: 1, depth: 2, seed: 7 };
    }
    return out;
}

function renderScene(name, sc, index) {
    const blob = exportScene(sc.test);
    fs.writeFileSync(path.join(outdir, name + ".jsrt"), blob);
    if (sc.no_render) return;
    const PixelBuffer = C("PixelBuffer"), Tex = C("TextureMaterialColor");
    const colors = new Float32Array(W * H * 4).fill(NaN);
    const lens = new Set();
    const pb = new PixelBuffer(W, H);
    const origSet = PixelBuffer.prototype.setColor;
    pb.setColor = function (x, y, color) {
        const i = y * W + x;
        for (let k = 0; k < 4; ++k) colors[4 * i + k] = k < color.length ? color[k] : NaN;
        lens.add(color.length);
        return origSet.call(this, x, y, color);
    };
    const ctl = installKeyedRng(sc.seed);
    ctl.startSequence(sampleOrder(sc.kind, W, H, sc.spp));
    // recorder: texture evaluations of primary hits (inside the root World.color call: two frames on the stack)
    const origColor = Tex.prototype.color;
    const primaryPixels = new Set();
    let primaryCalls = 0, primaryOutside = 0, calls = 0;
    Tex.prototype.color = function (data) {
        ++calls;
        if (ctl.stack.length === 2) {
            primaryPixels.add(ctl.cur[0]);
            ++primaryCalls;
            const u = data.UV[0], v = data.UV[1];
            if (!(u >= 0 && u <= 1 && v >= 0 && v <= 1)) ++primaryOutside;
        }
        return origColor.call(this, data);
    };
    try {
        sc.test.renderer.render(pb, 0, false, 0, 1);  // (a throw ends the generator: the first precondition)
    } finally {
        Tex.prototype.color = origColor;
    }
    if (lens.size !== 1 || !lens.has(3)) throw new Error(`${name}: setColor saw colour lengths ${[...lens]}`);
    if (primaryPixels.size * 4 < W * H) throw new Error(`${name}: only ${primaryPixels.size} of ${W * H} pixels' primary hits are textured`);
    if (primaryOutside * 10 < primaryCalls) throw new Error(`${name}: only ${primaryOutside} of ${primaryCalls} primary texture calls have a UV outside [0, 1]^2`);
    fs.writeFileSync(path.join(outdir, name + ".rgba"), Buffer.from(pb.imgdata.data.buffer));
    fs.writeFileSync(path.join(outdir, name + ".f32"), Buffer.from(colors.buffer));
    index[name] = { width: W, height: H, kind: sc.kind, spp: sc.spp, depth: sc.depth, seed: sc.seed, draws: ctl.draws,
                    color_calls: ctl.colorCalls, texture_calls: calls, primary_textured_pixels: primaryPixels.size,
                    primary_texture_calls: primaryCalls, primary_calls_outside_unit_uv: primaryOutside };
    console.log(`${name}: blob ${blob.length} B, ${primaryPixels.size}/${W * H} textured primary pixels, ` +
                `${primaryOutside}/${primaryCalls} primary calls outside [0,1]^2, ${calls} texture calls`);
}

makeKats();
const index = {};
for (const [name, sc] of Object.entries(scenes())) renderScene(name, sc, index);
fs.writeFileSync(path.join(outdir, "scenes.json"), JSON.stringify(index, null, 1));
