"use strict";
/*
 * TEST INFRASTRUCTURE ONLY.  Generates tests/golden/posuv/ by running the REFERENCE's own code (loaded at run time
 * by oracle/refharness/load_reference.js; nothing of it is copied): five 32x24 scenes whose surfaces get their UV
 * from PositionalUVMaterial (src/materials.js:177-193), rendered by the reference's renderers with the keyed RNG
 * (oracle/refharness/keyed_rng.js), each stored as its exported blob (jsraytracer_amd/js/scene_blob.js), the
 * reference's RGBA8 and f32 image, and -- for 256 primary and 512 random rays -- the data.UV the base material's
 * color() received (after every wrapper ran), recorded by replacing color() of the five non-wrapper Material
 * classes, the method of oracle/refharness/make_material_kats.js.  Scenes are built here from the reference's
 * classes; the output is data only.
 *
 *   node tools/make_posuv_fixtures.js <outdir>        (tools/make_posuv_fixtures.sh)
 *
 * It also writes <outdir>/../mtlmap/ (the MTL texture-map scene, described at mtlmap() below): scene.obj, scene.mtl,
 * the two images as raw RGBA8, skel.jsrt (the tree built from the first triangle only: the input of the native
 * ingest), full.jsrt (the reference-built scene exported), simple / incremental .rgba / .f32 and scenes.json.
 *
 * <scene>.jsrt / .rgba / .f32   as tools/make_texture_fixtures.js writes them
 * <scene>.json                  JSON.stringify(new Serializer(test).plain()), for the scenes without a texture (a
 *                               TextureMaterialColor does not survive the reference's own JSON round trip)
 * <scene>.uv.json               {n, n_primary, rays (base64 f32 n x 6), uv (f32 n x 2, NaN = none), has_uv (i32),
 *                               position (f32 n x 4: data.position), map (i32: index into scenes.json's mappings of
 *                               the innermost wrapper that ran, -1 none)}
 * scenes.json                   per scene the render parameters, the counts below and `mappings`
 *
 * The generator fails unless, per scene: the reference threw nothing; at least a quarter of the primary hits are on
 * wrapped materials; at least a tenth of the recorded UVs lie outside [0, 1]^2; every geometry kind the scene is
 * there for is hit by a recorded ray under a wrapper.
 */
const fs = require("fs");
const path = require("path");
const { refClass } = require("../oracle/refharness/load_reference");
const { installKeyedRng, sampleOrder } = require("../oracle/refharness/keyed_rng");
const { exportScene } = require("../jsraytracer_amd/js/scene_blob");

const C = (n) => refClass(n);
const outdir = path.resolve(process.argv[2] || "tests/golden/posuv");
fs.mkdirSync(outdir, { recursive: true });

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
const b64 = (typed) => Buffer.from(typed.buffer, typed.byteOffset, typed.byteLength).toString("base64");

const W = 32, H = 24;
function scenes() {
    const Vec = C("Vec"), Mat4 = C("Mat4"), Prim = C("Primitive"), Tex = C("TextureMaterialColor");
    const Phong = C("PhongMaterial"), Fresnel = C("FresnelPhongMaterial"), Path = C("PhongPathTracingMaterial");
    const SolidMat = C("SolidColorMaterial"), Transparent = C("TransparentMaterial"), PosUV = C("PositionalUVMaterial");
    const Scaled = C("ScaledMaterialColor"), Checker = C("CheckerboardMaterialColor");
    const Point = C("SimplePointLight"), World = C("World"), Cam = C("PerspectiveCamera");
    const rotX = (a) => Mat4.rotation(a, Vec.of(1, 0, 0)), rotY = (a) => Mat4.rotation(a, Vec.of(0, 1, 0));
    const checks = (a, b) => new Checker(Vec.of(...a), Vec.of(...b));
    const out = {};

    // flat: SimpleRenderer, a point light, depth 2 (the LDS-staged k_shade).  flat_plain: the same scene with a
    // checkerboard where the box's texture is, so that its Serializer JSON exists: the nested pair, the shared
    // mapping shapes (3/3/3, 4/3/4, 4/4/3) and every base kind through the JSON reader
    for (const [name, textured] of [["flat", true], ["flat_plain", false]]) {
        const floor = new PosUV(new Phong(Vec.of(1, 1, 1), checks([0.75, 0.75, 0.75], [0.125, 0.125, 0.25]), 0.5, 0.25, 10, 0.125));
        const boxTex = textured ? new Tex(image(8, 6, 11), "bilinear", false, true) : checks([0.5, 1, 0.25], [1, 0.25, 0.5]);
        const box = new PosUV(new Phong(Vec.of(1, 1, 1), 0.125, boxTex, 0.25, 20),
                              Vec.of(0.25, -0.5, 1.5, 1), Vec.of(0.5, 0.25, -0.125), Vec.of(-0.25, 0.5, 0.375, 0.75));
        const ball = new PosUV(new Phong(Vec.of(1, 0.75, 0.5), checks([1, 1, 1], [0.25, 0.5, 0.25]), 0.5, 0.5, 30),
                               Vec.of(0, 0, 0), Vec.of(2, 0, 0.5), Vec.of(0, 2.5, 0));
        const twice = new PosUV(new PosUV(new Phong(Vec.of(1, 1, 1), checks([1, 0.25, 0.25], [0.25, 0.25, 1]), 0.5, 0, 5),
                                          Vec.of(1, 2, 3), Vec.of(1.5, 0, 0), Vec.of(0, 1.5, 0)),
                                Vec.of(-4, 0, 9, 1), Vec.of(0, 0, 7, 0), Vec.of(0.125, 0, 0));
        const solid = new PosUV(new SolidMat(checks([1, 1, 0], [0, 0.5, 0.5])), Vec.of(0, 0, 0), Vec.of(3, 0, 0), Vec.of(0, 3, 0));
        const glass = new PosUV(new Transparent(checks([1, 0.5, 0], [0, 0.25, 0.5]), 0.5), Vec.of(0.5, 0.5, 0.5, 1), Vec.of(0, 4, 0, 2), Vec.of(4, 0, 0));
        const objects = [
            new Prim(new (C("Plane"))(), floor, Mat4.translation([0, -1, 0]).times(rotX(-Math.PI / 2))),
            new Prim(new (C("UnitBox"))(), box, Mat4.translation([-1.75, -0.25, -5]).times(rotY(0.5)).times(Mat4.scale(1.5))),
            new Prim(new (C("Sphere"))(), ball, Mat4.translation([1.25, 0, -4.5])),
            new Prim(new (C("Square"))(), twice, Mat4.translation([0, 1.5, -7]).times(Mat4.scale([3, 2, 1]))),
            new Prim(new (C("Circle"))(), solid, Mat4.translation([3, 1.25, -6]).times(Mat4.scale(1.25))),
            new Prim(new (C("Square"))(), glass, Mat4.translation([0.25, -0.25, -3]).times(Mat4.scale(1.25))),
        ];
        const world = new World(objects, [new Point(Vec.of(3, 5, 0, 1), Vec.of(1, 1, 1), 150)], Vec.of(0.125, 0.125, 0.25));
        out[name] = { test: { renderer: new (C("SimpleRenderer"))(world, new Cam(Math.PI / 3, W / H, Mat4.translation([0, 0.5, 0]).times(rotX(-0.2))), 2), width: W, height: H },
                     kind: 0, spp: 1, depth: 2, seed: 5, kinds: ["SimplePlane", "AABB", "Sphere", "Square", "Circle"], json: !textured };
    }
    {   // box: a closed box of PhongPathTracing walls with a textured diffusivity under the wrapper, one Square area
        //      light of 4 samples; Incremental, 4 spp, depth 3 (the hybrid chain, k_shadow_node, the HAND_DIFF plane)
        const wallTex = new Tex(image(7, 5, 21), "bilinear", false, false);
        const wrapped = (base, tint, origin, ua, va) => new PosUV(new Path(Vec.of(...base), 0, tint), origin, ua, va);
        const objects = [
            new Prim(new (C("Square"))(), wrapped([1, 1, 1], wallTex, Vec.of(0, 0, 0), Vec.of(0.25, 0, 0), Vec.of(0, 0.25, 0)),
                     Mat4.translation([0, 5, -5]).times(Mat4.scale([10, 10, 1]))),                              // back
            new Prim(new (C("Square"))(), new Path(Vec.of(1, 1, 1), 0, 0.5), Mat4.translation([0, 5, 16]).times(Mat4.scale([10, 10, 1]))),
            new Prim(new (C("Square"))(), wrapped([1, 0.125, 0.125], new Scaled(wallTex, 0.5), Vec.of(0, 0, 0, 1), Vec.of(0, 0.125, 0.0625), Vec.of(0, 0, 0.25)),
                     Mat4.translation([5, 5, 5]).times(Mat4.scale([1, 10, 22])).times(rotY(Math.PI / 2))),
            new Prim(new (C("Square"))(), new Path(Vec.of(0.125, 1, 0.125), 0, 0.5),
                     Mat4.translation([-5, 5, 5]).times(Mat4.scale([1, 10, 22])).times(rotY(-Math.PI / 2))),
            new Prim(new (C("Square"))(), wrapped([1, 1, 1], wallTex, Vec.of(1, 0, 2), Vec.of(0.125, 0, 0.125), Vec.of(-0.125, 0, 0.125)),
                     Mat4.translation([0, 0, 5]).times(Mat4.scale([10, 1, 22])).times(rotX(Math.PI / 2))),       // floor
            new Prim(new (C("Square"))(), new Path(Vec.of(1, 1, 1), 0, 0.5), Mat4.translation([0, 10, 5]).times(Mat4.scale([10, 1, 22])).times(rotX(Math.PI / 2))),
            new Prim(new (C("Sphere"))(), new Path(Vec.of(1, 1, 1), 0, 0.125, 0.75, 10, 2), Mat4.translation([-2.5, 1.5, 0]).times(Mat4.scale(1.5))),
        ];
        const light = new (C("RandomSampleAreaLight"))(new (C("Square"))(),
            Mat4.translation([0, 9.5, 0]).times(rotX(-Math.PI / 2)).times(Mat4.scale([2, 2, 1])), Vec.of(1, 1, 1), 600, 4);
        const world = new World(objects, [light]);
        out.box = { test: { renderer: new (C("IncrementalMultisamplingRenderer"))(world, new Cam(Math.PI / 4, W / H, Mat4.translation([0, 5, 15])), 4, 3), width: W, height: H },
                    kind: 1, spp: 4, depth: 3, seed: 9, kinds: ["Square"] };
    }
    {   // mesh: a BVH of 40 triangles without UVs under a wrapper with a texture, inside a transformed Aggregate
        //       (world position and local position differ)
        const meshTex = new Tex(image(8, 8, 31), "bilinear", false, false);
        const mat = new PosUV(new Fresnel(Vec.of(1, 1, 1), new Scaled(meshTex, 0.5), new Scaled(meshTex, Vec.of(0.5, 0.75, 1)), 0.25, 10, 1.5),
                              Vec.of(0.5, 0.25, -6, 1), Vec.of(0.375, 0.125, 0), Vec.of(-0.125, 0.375, 0.25));
        const nx = 5, ny = 4, tris = [];
        const P = (i, j) => Vec.of(-2.5 + i, -2 + j, 0.25 * Math.sin(1.5 * i) * Math.cos(1.25 * j), 1);
        for (let i = 0; i < nx; ++i)
            for (let j = 0; j < ny; ++j) {
                const q = [[i, j], [i + 1, j], [i + 1, j + 1], [i, j + 1]];
                for (const t of [[0, 1, 2], [0, 2, 3]]) tris.push(new Prim(new (C("Triangle"))(t.map(k => P(...q[k]))), mat));
            }
        const agg = new (C("Aggregate"))([C("BVHAggregate").build(tris)], Mat4.translation([0.25, 0, -6]).times(rotY(0.3)).times(Mat4.scale(1.125)));
        const world = new World([agg], [new Point(Vec.of(2, 3, 2, 1), Vec.of(1, 1, 1), 120)], Vec.of(0.25, 0.125, 0.125));
        out.mesh = { test: { renderer: new (C("SimpleRenderer"))(world, new Cam(Math.PI / 4, W / H, Mat4.translation([0, 0, 0.5])), 3), width: W, height: H },
                     kind: 0, spp: 1, depth: 3, seed: 3, kinds: ["Triangle"] };
    }
    {   // sdf: SDF primitives with a basecolor under a wrapper with a checkerboard
        const mat = new PosUV(new Phong(Vec.of(1, 1, 1), checks([1, 1, 1], [0.25, 0.25, 0.25]), 0.5, 0.25, 10),
                              Vec.of(0.125, 0.25, 0.375, 1), Vec.of(3, 0, 1), Vec.of(0, 3, -1, 0));
        const sdf = new (C("UnionSDF"))(new (C("SphereSDF"))(1, Vec.of(1, 0.5, 0.25)),
                                        new (C("TransformSDF"))(new (C("BoxSDF"))(0.5, Vec.of(0.25, 0.5, 1)),
                                                                new (C("SDFMatrixTransformer"))(Mat4.translation([1.25, 0.25, 0]))));
        const objects = [new Prim(new (C("SDFGeometry"))(sdf), mat, Mat4.translation([-0.25, 0, -4]).times(rotY(0.4)).times(Mat4.scale(1.25)))];
        const world = new World(objects, [new Point(Vec.of(3, 4, 1, 1), Vec.of(1, 1, 1), 100)], Vec.of(0.125, 0.25, 0.125));
        out.sdf = { test: { renderer: new (C("SimpleRenderer"))(world, new Cam(Math.PI / 4, W / H, Mat4.translation([0, 0, 0.5])), 2), width: W, height: H },
                    kind: 0, spp: 1, depth: 2, seed: 7, kinds: ["SDFGeometry"], json: true };
    }
    return out;
}

// data.UV as the base material's color() receives it, for 256 primary and 512 random rays
function recordUV(name, sc, entry) {
    const Vec = C("Vec"), Ray = C("Ray"), PosUV = C("PositionalUVMaterial");
    const world = sc.test.renderer.world, cam = sc.test.renderer.camera;
    const r = rng32(0xC0FFEE ^ sc.seed), rays = [];
    for (let j = 0; j < 16; ++j)
        for (let i = 0; i < 16; ++i) rays.push(cam.getRayForPixel((i + 0.5) / 8 - 1, (j + 0.5) / 8 - 1));
    const nPrimary = rays.length;
    for (let k = 0; k < 512; ++k) {
        const ray = cam.getRayForPixel(2.5 * r() - 1.25, 2.5 * r() - 1.25);
        rays.push(new Ray(ray.origin.plus(Vec.of(r() - 0.5, r() - 0.5, r() - 0.5, 0)), ray.direction));
    }
    const n = rays.length;
    const RR = new Float32Array(6 * n), UV = new Float32Array(2 * n).fill(NaN), HAS = new Int32Array(n),
          POS = new Float32Array(4 * n).fill(NaN), MAP = new Int32Array(n).fill(-1);
    const bases = ["SolidColorMaterial", "TransparentMaterial", "PhongMaterial", "FresnelPhongMaterial", "PhongPathTracingMaterial"].map(C);
    const saved = bases.map(c => Object.getOwnPropertyDescriptor(c.prototype, "color"));
    const wrapColor = PosUV.prototype.color;
    const mappings = [], mapOf = new Map();
    let captured = null, inner = null;
    for (const c of bases) c.prototype.color = function (data) { captured = data; return Vec.of(0, 0, 0); };
    PosUV.prototype.color = function (data, w, d) { inner = this; return wrapColor.call(this, data, w, d); };  // the last to run is the innermost
    let hits = 0, wrappedPrimary = 0, primaryHits = 0, outside = 0, recorded = 0;
    const kinds = new Set();
    try {
        rays.forEach((ray, k) => {
            for (let i = 0; i < 3; ++i) { RR[6 * k + i] = ray.origin[i]; RR[6 * k + 3 + i] = ray.direction[i]; }
            const q = new Ray(Vec.of(RR[6 * k], RR[6 * k + 1], RR[6 * k + 2], 1), Vec.of(RR[6 * k + 3], RR[6 * k + 4], RR[6 * k + 5], 0));
            captured = null; inner = null;
            const h = world.cast(q);
            world.color(q, 1);
            if (!captured) return;
            ++hits;
            if (k < nPrimary) ++primaryHits;
            for (let i = 0; i < 4; ++i) POS[4 * k + i] = captured.position[i];
            if (captured.UV) {
                UV[2 * k] = captured.UV[0]; UV[2 * k + 1] = captured.UV[1]; HAS[k] = 1;
                ++recorded;
                if (!(captured.UV[0] >= 0 && captured.UV[0] <= 1 && captured.UV[1] >= 0 && captured.UV[1] <= 1)) ++outside;
            }
            if (inner) {
                if (k < nPrimary) ++wrappedPrimary;
                kinds.add(h.object.geometry.constructor.name === "UnitBox" ? "AABB" :
                          h.object.geometry.constructor.name === "Plane" ? "SimplePlane" : h.object.geometry.constructor.name);
                if (!mapOf.has(inner)) {
                    mapOf.set(inner, mappings.length);
                    mappings.push({ origin: Array.from(inner.origin), u_axis: Array.from(inner.u_axis), v_axis: Array.from(inner.v_axis) });
                }
                MAP[k] = mapOf.get(inner);
            }
        });
    } finally {
        PosUV.prototype.color = wrapColor;
        bases.forEach((c, i) => { if (saved[i]) Object.defineProperty(c.prototype, "color", saved[i]); else delete c.prototype.color; });
    }
    if (wrappedPrimary * 4 < primaryHits || primaryHits === 0) throw new Error(`${name}: only ${wrappedPrimary} of ${primaryHits} primary hits are on wrapped materials`);
    if (outside * 10 < recorded) throw new Error(`${name}: only ${outside} of ${recorded} recorded UVs lie outside [0, 1]^2`);
    for (const kd of sc.kinds) if (!kinds.has(kd)) throw new Error(`${name}: no recorded ray hits a wrapped ${kd} (hit: ${[...kinds]})`);
    fs.writeFileSync(path.join(outdir, name + ".uv.json"), JSON.stringify(
        { n, n_primary: nPrimary, rays: b64(RR), uv: b64(UV), has_uv: b64(HAS), position: b64(POS), map: b64(MAP) }));
    Object.assign(entry, { mappings, uv_rays: n, uv_hits: hits, uv_recorded: recorded, uv_outside_unit: outside,
                           primary_hits: primaryHits, primary_wrapped: wrappedPrimary, wrapped_kinds: [...kinds].sort() });
    console.log(`${name}: ${hits}/${n} rays hit, ${wrappedPrimary}/${primaryHits} primary hits wrapped, ${outside}/${recorded} UVs outside [0,1]^2, kinds ${[...kinds]}`);
}

function renderScene(name, sc, index) {
    const blob = exportScene(sc.test);
    fs.writeFileSync(path.join(outdir, name + ".jsrt"), blob);
    if (sc.json) fs.writeFileSync(path.join(outdir, name + ".json"), JSON.stringify(new (C("Serializer"))(sc.test).plain()), "utf8");
    const PixelBuffer = C("PixelBuffer");
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
    const entry = { width: W, height: H, kind: sc.kind, spp: sc.spp, depth: sc.depth, seed: sc.seed, json: !!sc.json };
    recordUV(name, sc, entry);  // (before the keyed RNG is installed: no draw happens up to Material.color)
    const ctl = installKeyedRng(sc.seed);
    ctl.startSequence(sampleOrder(sc.kind, W, H, sc.spp));
    sc.test.renderer.render(pb, 0, false, 0, 1);  // (a throw ends the generator: the first precondition)
    if (lens.size !== 1 || !lens.has(3)) throw new Error(`${name}: setColor saw colour lengths ${[...lens]}`);
    fs.writeFileSync(path.join(outdir, name + ".rgba"), Buffer.from(pb.imgdata.data.buffer));
    fs.writeFileSync(path.join(outdir, name + ".f32"), Buffer.from(colors.buffer));
    index[name] = Object.assign(entry, { draws: ctl.draws, color_calls: ctl.colorCalls });
    console.log(`${name}: blob ${blob.length} B, ${ctl.colorCalls} World.color calls`);
}

const index = {};
for (const [name, sc] of Object.entries(scenes())) renderScene(name, sc, index);
fs.writeFileSync(path.join(outdir, "scenes.json"), JSON.stringify(index, null, 1));

// ---- MTL texture maps (tests/golden/mtlmap/) -----------------------------------------------------------------
// An OBJ and MTL of this project's own -- a UV-mapped box on a ground quad, 14 triangles, two materials, two
// textures: `crate` has map_Kd with Kd and map_Ks with Ks, `ground` has map_Ka alone -- built by the reference's own
// loadObjFile / parseMtlFile (objloader.js:58-247).  fetch / createImageBitmap / OffscreenCanvas are stubbed so that
// loadTexture and TextureMaterialColor.fromBitmap (objloader.js:33-40, materials.js:91-96) receive the seeded images.
const OBJ_TEXT = `# a box on a ground quad
mtllib scene.mtl
v -1 0 -1
v 1 0 -1
v 1 0 1
v -1 0 1
v -1 1.5 -1
v 1 1.5 -1
v 1 1.5 1
v -1 1.5 1
v -4 0 -4
v 4 0 -4
v 4 0 4
v -4 0 4
vt 0 0
vt 1 0
vt 1 1
vt 0 1
vt -0.5 -0.5
vt 1.5 -0.5
vt 1.5 1.5
vt -0.5 1.5
usemtl crate
f 4/1 3/2 7/3 8/4
f 3/1 2/2 6/3 7/4
f 2/1 1/2 5/3 6/4
f 1/1 4/2 8/3 5/4
f 8/5 7/6 6/7 5/8
f 1/1 2/2 3/3 4/4
usemtl ground
f 12/5 11/6 10/7 9/8
`;
const MTL_TEXT = `# two materials, two textures
newmtl crate
Ka 0.125 0.125 0.125
Kd 0.75 0.5 1
map_Kd -clamp on wood.png
Ks 0.5 0.5 0.5
map_Ks spec.png
Ns 20
Ni 1.5
illum 2

newmtl ground
map_Ka wood.png
Kd 0.25 0.5 0.25
`;
async function mtlmap() {
    const dir = path.join(outdir, "..", "mtlmap");
    fs.mkdirSync(dir, { recursive: true });
    fs.writeFileSync(path.join(dir, "scene.obj"), OBJ_TEXT);
    fs.writeFileSync(path.join(dir, "scene.mtl"), MTL_TEXT);
    const images = { "wood.png": image(8, 8, 41), "spec.png": image(5, 3, 42) };
    global.fetch = (filename) => Promise.resolve({ ok: true, blob: () => Promise.resolve({ name: path.basename(filename) }) });
    global.createImageBitmap = (blob) => {
        if (!images[blob.name]) throw new Error("no image " + blob.name);
        return Promise.resolve({ width: images[blob.name].width, height: images[blob.name].height, img: images[blob.name] });
    };
    global.OffscreenCanvas = class {
        constructor(w, h) { this.width = w; this.height = h; }
        getContext() { const c = { drawImage(b) { c.bitmap = b; }, getImageData() { return c.bitmap.img; } }; return c; }
    };
    const Vec = C("Vec"), Mat4 = C("Mat4"), World = C("World"), Cam = C("PerspectiveCamera"), BVH = C("BVHAggregate");
    const fallback = new (C("PhongMaterial"))(Vec.of(1, 0, 1), 0.5, 0.5);
    const make = async (first) => {
        const tris = await new Promise((resolve) => loadObjFile(path.join(dir, "scene.obj"), fallback, resolve, Mat4.identity(), 0.00001));
        const agg = BVH.build(first ? [tris[0]] : tris, Mat4.translation([0, -1, -6]).times(Mat4.rotation(0.6, Vec.of(0, 1, 0))));
        const world = new World([agg], [new (C("SimplePointLight"))(Vec.of(3, 4, -1, 1), Vec.of(1, 1, 1), 60)], Vec.of(0.125, 0.125, 0.25));
        const cam = new Cam(Math.PI / 4, W / H, Mat4.translation([0, 1.5, 0]).times(Mat4.rotation(-0.3, Vec.of(1, 0, 0))));
        return { test: { renderer: new (C("SimpleRenderer"))(world, cam, 2), width: W, height: H }, world, cam, n: tris.length };
    };
    const full = await make(false), skel = await make(true);
    if (full.n !== 14) throw new Error("mtlmap: expected 14 triangles, got " + full.n);
    fs.writeFileSync(path.join(dir, "full.jsrt"), exportScene(full.test));
    fs.writeFileSync(path.join(dir, "skel.jsrt"), exportScene(skel.test));
    const idx = { textures: {}, triangles: full.n, renders: {} };
    for (const [name, img] of Object.entries(images)) {
        const f = name + ".rgba8";
        fs.writeFileSync(path.join(dir, f), Buffer.from(img.data.buffer));
        idx.textures[name] = { file: f, width: img.width, height: img.height };
    }
    const Tex = C("TextureMaterialColor"), PixelBuffer = C("PixelBuffer");
    for (const [name, kind, spp, seed] of [["simple", 0, 1, 11], ["incremental", 1, 4, 12]]) {
        const R = kind === 0 ? full.test.renderer : new (C("IncrementalMultisamplingRenderer"))(full.world, full.cam, spp, 2);
        const colors = new Float32Array(W * H * 4).fill(NaN), lens = new Set();
        const pb = new PixelBuffer(W, H), origSet = PixelBuffer.prototype.setColor;
        pb.setColor = function (x, y, color) {
            for (let k = 0; k < 4; ++k) colors[4 * (y * W + x) + k] = k < color.length ? color[k] : NaN;
            lens.add(color.length);
            return origSet.call(this, x, y, color);
        };
        const ctl = installKeyedRng(seed);
        ctl.startSequence(sampleOrder(kind, W, H, spp));
        const origColor = Tex.prototype.color;
        const used = new Set();
        let calls = 0;
        Tex.prototype.color = function (data) { ++calls; used.add(this); return origColor.call(this, data); };
        try { R.render(pb, 0, false, 0, 1); } finally { Tex.prototype.color = origColor; }
        if (lens.size !== 1 || !lens.has(3)) throw new Error(`mtlmap ${name}: setColor saw colour lengths ${[...lens]}`);
        if (used.size !== 2 || calls * 4 < W * H) throw new Error(`mtlmap ${name}: ${used.size} textures sampled in ${calls} calls`);
        fs.writeFileSync(path.join(dir, name + ".rgba"), Buffer.from(pb.imgdata.data.buffer));
        fs.writeFileSync(path.join(dir, name + ".f32"), Buffer.from(colors.buffer));
        idx.renders[name] = { width: W, height: H, kind, spp, depth: 2, seed, draws: ctl.draws, color_calls: ctl.colorCalls, texture_calls: calls };
        console.log(`mtlmap ${name}: ${calls} texture calls, ${ctl.colorCalls} World.color calls`);
    }
    fs.writeFileSync(path.join(dir, "scenes.json"), JSON.stringify(idx, null, 1));
}
mtlmap().catch((e) => { console.error(e); process.exit(1); });
