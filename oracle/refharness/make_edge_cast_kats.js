"use strict";
/*
 * TEST INFRASTRUCTURE ONLY.  Edge-case known answers for World.cast, computed by the reference itself
 * (vm-loaded by load_reference.js), beside make_cast_kats.js's generic rays: rays at the places where one
 * comparison decides the reference's answer (world.js:11 strict `<` and first-wins order, geometry.js:194
 * the slab's |d_i| > 1e-7, geometry.js:374 barycentrics in [0, 1], aggregates.js:209 `min <= ret.distance`).
 * Every ray is derived generically from what the reference exposes (World.cast, getBoundingBox, the
 * aggregates' objects / kdtree, Triangle.ps), stored as the f32 values its Vec holds.
 *
 * Set kinds (each as a closest cast, transparent objects included, and as "<kind>.shadow": minD 0.0001,
 * maxD 1, shadow casters only -- except where the kind fixes its own range):
 *   from_hit      groups of 4 consecutive rays sharing an origin P = a reference hit point, minD 0 and 0.0001
 *                 ("from_hit", "from_hit.eps", "from_hit.shadow");
 *   to_hit        segments Q -> P (hit at t ~ 1), d scaled by 1, 1 +- 2^-23, 1 +- 1e-4; maxD 1;
 *   lim_tie       rays of known hit distance t recast with maxD, then minD, in {t, next double above, below}:
 *                 per-ray ranges (minD_each / maxD_each, f64); ".shadow" takes t from the shadow-casters cast;
 *   axis          grid origins, direction components from {+-0, +-1, +-1e-7 and its f32 neighbours, +-1e-8, +-2e-7};
 *   box_features  rays at the corners, edge midpoints and face centres of the boxes of objects, aggregate
 *                 members and BVH nodes (depth <= 4), and rays running in their face planes and along edges;
 *   tri_features  (BVH scenes) rays at triangle vertices, edge midpoints and centroids from both sides, and
 *                 rays in the triangle's plane; "aim" is the triangle aimed at (OBJS index);
 *   scaled        a subset with d x 1e-3 and x 1e3, and origins ~1e3 scene extents away aimed at features.
 *
 *   node oracle/refharness/make_edge_cast_kats.js <outdir> <scene>...
 * writes <outdir>/<scene>.json: {scene, blob_sha256, sets: [{name, kind, minD, maxD, transp, n, dropped,
 *   rays | rays_of (the name of the set whose rays these are), t, obj, [minD_each, maxD_each], [aim]}]}
 * (base64 as make_cast_kats.js).  A ray whose reference distance is NaN in any cast of its kind is dropped
 * (`dropped`, at most 1 %).  The fixture conditions (tests/test_oracle_casts_edge.py asserts them again) are
 * asserted here.
 */
const fs = require("fs");
const path = require("path");
const crypto = require("crypto");
const { loadScene, refClass } = require("./load_reference");
const { SceneBlobWriter } = require("../../jsraytracer_amd/js/scene_blob");

let s = 0x13579bd;
function r() { s = (Math.imul(s, 1103515245) + 12345) >>> 0; return s / 4294967296; }
const ri = (n) => Math.min(n - 1, Math.floor(r() * n));
const b64 = (typed) => Buffer.from(typed.buffer, typed.byteOffset, typed.byteLength).toString("base64");
const f32 = Math.fround;

const cvt = new DataView(new ArrayBuffer(8));
function nextDouble(x, up) {  // the neighbouring double of a finite positive x
    cvt.setFloat64(0, x);
    const b = cvt.getBigUint64(0) + (up ? 1n : -1n);
    cvt.setBigUint64(0, b);
    return cvt.getFloat64(0);
}
function nextF32(x, up) {     // the neighbouring f32 of a finite positive f32 x
    cvt.setFloat32(0, x);
    cvt.setUint32(0, cvt.getUint32(0) + (up ? 1 : -1));
    return cvt.getFloat32(0);
}

const add = (a, b) => [a[0] + b[0], a[1] + b[1], a[2] + b[2]];
const sub = (a, b) => [a[0] - b[0], a[1] - b[1], a[2] - b[2]];
const mul = (a, k) => [a[0] * k, a[1] * k, a[2] * k];
const len = (a) => Math.hypot(a[0], a[1], a[2]);
const cross = (a, b) => [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]];
const unit = (a) => mul(a, 1 / (len(a) || 1));

function sample(list, n) {    // n of list, in order, chosen by r()
    if (list.length <= n) return list;
    const idx = list.map((_, i) => i);
    for (let i = 0; i < n; ++i) { const j = i + ri(idx.length - i); [idx[i], idx[j]] = [idx[j], idx[i]]; }
    return idx.slice(0, n).sort((a, b) => a - b).map(i => list[i]);
}

const N = { hits: 400, from_hit: 40, to_hit: 36, lim_tie: 30, axis: 150, box: 170, tri: 170, scaled: 140 };

async function main() {
    const argv = process.argv.slice(2);
    const outdir = path.resolve(argv[0]);
    fs.mkdirSync(outdir, { recursive: true });
    const Vec = refClass("Vec"), Ray = refClass("Ray"), Mat4 = refClass("Mat4");
    for (const name of argv.slice(1)) {
        const test = await loadScene(name);
        const w = new SceneBlobWriter();
        const blob = w.build(test);
        const world = test.renderer.world;
        const box = world.getFiniteBoundingBox();
        const lo = [0, 1, 2].map(i => box.center[i] - 1.5 * box.half_size[i]);
        const ext = [0, 1, 2].map(i => 3 * box.half_size[i]);
        const extent = len(ext);
        const point = () => [lo[0] + r() * ext[0], lo[1] + r() * ext[1], lo[2] + r() * ext[2]];
        const dir = () => { const th = 2 * Math.PI * r(), z = 2 * r() - 1, q = Math.sqrt(1 - z * z); return [q * Math.cos(th), q * Math.sin(th), z]; };
        const objOf = (o) => (o == null ? -1 : w.maps.obj.get(o));
        const mk = (o, d, aim) => {
            const ray = new Ray(Vec.of(o[0], o[1], o[2], 1), Vec.of(d[0], d[1], d[2], 0));
            ray.aim = aim === undefined ? -1 : aim;
            return ray;
        };
        const usable = (ray) => ray.origin.every(isFinite) && ray.direction.every(isFinite) &&
                                (ray.direction[0] != 0 || ray.direction[1] != 0 || ray.direction[2] != 0);
        const xf = (M, p) => Array.from(M.times(Vec.of(p[0], p[1], p[2], 1))).slice(0, 3);

        // ---- what the reference exposes: boxes (corner points in world space) and triangles
        const boxes = [], tris = [];
        const addBox = (aabb, M) => {
            if (!aabb.isFinite() || !(aabb.half_size[0] + aabb.half_size[1] + aabb.half_size[2] > 0)) return;
            boxes.push(aabb.getCorners().map(c => xf(M, c)));
        };
        const bvhNodes = (node, M, depth) => {
            if (!node || depth > 4) return;
            addBox(node.aabb, M);
            bvhNodes(node.lesser_node, M, depth + 1);
            bvhNodes(node.greater_node, M, depth + 1);
        };
        const walk = (o, M, top) => {       // M: the frame o's bounding box is expressed in -> world
            addBox(o.getBoundingBox(), M);
            if (o.objects) {
                const Mo = M.times(o.getTransform());
                if (o.kdtree && o.kdtree.aabb) bvhNodes(o.kdtree, Mo, 0);
                for (const c of o.objects) walk(c, Mo, false);
            } else if (o.object) {
                walk(o.object, M.times(o.getTransform()), false);
            } else if (o.geometry && o.geometry.ps && o.geometry.ps.length == 3) {
                const Mo = M.times(o.getTransform());
                tris.push({ p: o.geometry.ps.map(p => xf(Mo, p)), obj: objOf(o) });
            }
        };
        // bound the walk of a big mesh: boxes of at most 64 members per aggregate are enough
        const walkTop = (o) => {
            if (o.objects && o.objects.length > 64) {
                const M = Mat4.identity(), Mo = M.times(o.getTransform());
                addBox(o.getBoundingBox(), M);
                if (o.kdtree && o.kdtree.aabb) bvhNodes(o.kdtree, Mo, 0);
                const keep = new Set(sample(o.objects.map((_, i) => i), 64));
                o.objects.forEach((c, i) => {
                    if (keep.has(i)) walk(c, Mo, false);
                    else if (c.geometry && c.geometry.ps && c.geometry.ps.length == 3)
                        tris.push({ p: c.geometry.ps.map(p => xf(Mo.times(c.getTransform()), p)), obj: objOf(c) });
                });
            } else walk(o, Mat4.identity(), true);
        };
        world.objects.forEach(walkTop);

        // ---- reference hit points
        const hits = [];
        for (let k = 0; k < 20 * N.hits && hits.length < N.hits; ++k) {
            const ray = mk(point(), dir());
            const h = world.cast(ray);
            if (h.object != null && isFinite(h.distance) && h.distance > 0) hits.push({ ray, t: h.distance, P: Array.from(ray.getPoint(h.distance)).slice(0, 3) });
        }
        if (hits.length < 100) throw new Error(name + ": too few reference hits");

        const sets = [];
        // One kind: its rays and the casts to run on them.  runs: [suffix, minD, maxD, transp]; a range given as
        // a function of the ray index makes a per-ray range.
        const emit = (kind, rays, runs, opt = {}) => {
            rays = rays.filter(usable);
            const res = runs.map(([suffix, minD, maxD, transp]) => rays.map((ray, k) => {
                const a = typeof minD == "function" ? minD(k) : minD, b = typeof maxD == "function" ? maxD(k) : maxD;
                const h = world.cast(ray, a, b, transp);
                return { t: h.distance, obj: objOf(h.object), a, b };
            }));
            const keep = rays.map((_, k) => res.every(rr => !Number.isNaN(rr[k].t)));
            const n = keep.filter(x => x).length, dropped = rays.length - n;
            if (dropped > 0.01 * rays.length) throw new Error(`${name}/${kind}: ${dropped} of ${rays.length} rays are NaN in the reference`);
            const R = new Float32Array(6 * n), A = new Int32Array(n);
            let j = 0;
            rays.forEach((ray, k) => {
                if (!keep[k]) return;
                for (let i = 0; i < 3; ++i) { R[6 * j + i] = ray.origin[i]; R[6 * j + 3 + i] = ray.direction[i]; }
                A[j++] = ray.aim;
            });
            runs.forEach(([suffix, minD, maxD, transp], ri_) => {
                const T = new Float64Array(n), O = new Int32Array(n), LA = new Float64Array(n), LB = new Float64Array(n);
                j = 0;
                res[ri_].forEach((x, k) => { if (keep[k]) { T[j] = x.t; O[j] = x.obj; LA[j] = x.a; LB[j] = x.b; ++j; } });
                const e = { name: kind + suffix, kind, minD: typeof minD == "function" ? null : minD,
                            maxD: typeof maxD == "function" ? null : (isFinite(maxD) ? maxD : "Infinity"), transp, n, dropped };
                if (typeof minD == "function") e.minD_each = b64(LA);
                if (typeof maxD == "function") e.maxD_each = b64(LB);
                if (ri_ == 0) e.rays = b64(R); else e.rays_of = kind + runs[0][0];
                e.t = b64(T); e.obj = b64(O);
                if (opt.aim && ri_ == 0) e.aim = b64(A);
                const nh = O.reduce((acc, o) => acc + (o >= 0), 0);
                if (transp && (nh < 50 || n - nh < 50)) throw new Error(`${name}/${e.name}: ${nh} hits, ${n - nh} misses (50 of each wanted)`);
                if (opt.check) opt.check(e, T, O, A);
                e.hits = nh;
                sets.push(e);
            });
            return rays.filter((_, k) => keep[k]);
        };
        const STD = [["", 0, Infinity, true], [".shadow", 0.0001, 1, false]];
        // n of the units (arrays of rays that stay together), so that the closest cast has hits and misses
        // enough in every scene: two fifths from those that miss most, two fifths from those that hit most, the rest at random
        const balance = (units, n, maxD = Infinity, minDs = [0]) => {
            units = sample(units.filter(u => u.every(usable)), units.length);
            if (units.length <= n) return units.flat();
            const score = new Map(units.map(u => [u, u.reduce((a, ray) => a + minDs.reduce((b, minD) => b + (world.cast(ray, minD, maxD, true).object != null), 0), 0) / u.length]));
            const third = Math.ceil(0.4 * n), picked = new Set(units.slice(0, n - 2 * third));
            const rest = () => units.filter(u => !picked.has(u));
            for (const u of rest().sort((a, b) => score.get(a) - score.get(b)).slice(0, third)) picked.add(u);
            for (const u of rest().sort((a, b) => score.get(b) - score.get(a)).slice(0, third)) picked.add(u);
            return units.filter(u => picked.has(u)).flat();
        };

        // ---- from_hit: 4 consecutive rays per origin P; half of the groups aim at random points (segments, as
        // shadow rays are), half have unit directions
        {
            const groups = [];
            for (const h of hits) {
                const seg = r() < 0.5;
                groups.push([0, 1, 2, 3].map(() => mk(h.P, seg ? sub(point(), h.P) : dir())));
            }
            emit("from_hit", balance(groups, N.from_hit, Infinity, [0, 0.0001]), [["", 0, Infinity, true], [".eps", 0.0001, Infinity, true], [".shadow", 0.0001, 1, false]]);
        }
        // ---- to_hit: Q -> P, the hit at t ~ 1
        {
            const groups = [];
            for (const h of hits) {
                const Q = r() < 0.5 ? Array.from(h.ray.origin).slice(0, 3) : point();
                const d = sub(h.P.map(f32), Q.map(f32));
                groups.push([1, 1 + 2 ** -23, 1 - 2 ** -23, 1 + 1e-4, 1 - 1e-4].map(k => mk(Q, mul(d, k))));
            }
            emit("to_hit", balance(groups, N.to_hit, 1), [["", 0, 1, true], [".shadow", 0.0001, 1, false]]);
        }
        // ---- lim_tie: the range's end on the hit distance itself
        for (const [suffix, transp] of [["", true], [".shadow", false]]) {
            const base = [];
            for (const h of hits) {
                const t = world.cast(h.ray, 0, Infinity, transp).distance;
                if (isFinite(t) && t > 1e-3) base.push({ ray: h.ray, t });
            }
            const rays = [], A = [], B = [];
            for (const b of sample(base, N.lim_tie)) {
                for (const lim of [b.t, nextDouble(b.t, true), nextDouble(b.t, false)]) { rays.push(b.ray); A.push(0); B.push(lim); }
                for (const lim of [b.t, nextDouble(b.t, true), nextDouble(b.t, false)]) { rays.push(b.ray); A.push(lim); B.push(Infinity); }
            }
            const check = (e, T, O) => {
                const h = O.filter(o => o >= 0).length;
                if (!(h > 0 && h < e.n)) throw new Error(`${name}/${e.name}: tied rays have ${h} hits of ${e.n}`);
            };
            if (rays.some(x => !usable(x))) throw new Error("lim_tie: unusable base ray");
            // transp = true must have 50 hits and 50 misses as every closest set; emit() checks that
            emit("lim_tie", rays, [[suffix, (k) => A[k], (k) => B[k], transp]], { check });
        }
        // ---- axis: zero and near-1e-7 direction components
        {
            const e7 = f32(1e-7), tiny = [0, -0, e7, -e7, nextF32(e7, true), -nextF32(e7, true), nextF32(e7, false), -nextF32(e7, false),
                                        1e-8, -1e-8, 2e-7, -2e-7];
            const comp = () => (r() < 0.4 ? (r() < 0.5 ? 1 : -1) : tiny[ri(tiny.length)]);
            const G = 5, rays = [];
            const grid = () => [0, 1, 2].map(i => box.center[i] + box.half_size[i] * (2 * ri(G) / (G - 1) - 1) * 1.25);
            while (rays.length < 4 * N.axis) {
                let d;
                const kind = rays.length % 3;
                if (kind == 0) { d = [0, 0, 0]; d[ri(3)] = comp() || 1; }                       // two exact zeros
                else if (kind == 1) { d = [comp() || 1, comp() || e7, comp() || -e7]; d[ri(3)] = r() < 0.5 ? 0 : -0; }  // one
                else d = [comp(), comp(), comp()];
                if (!d.some(x => Math.abs(x) == 1)) d[ri(3)] = r() < 0.5 ? 1 : -1;
                rays.push(mk(grid(), d));
            }
            emit("axis", balance(rays.map(x => [x]), N.axis), STD);
        }
        // ---- box_features
        const feat = [];    // kept for "scaled": {target, from}
        {
            const rays = [];
            const EDGES = [[0, 1], [2, 3], [4, 5], [6, 7], [0, 2], [1, 3], [4, 6], [5, 7], [0, 4], [1, 5], [2, 6], [3, 7]];
            const FACES = [[0, 1, 2, 3], [4, 5, 6, 7], [0, 1, 4, 5], [2, 3, 6, 7], [0, 2, 4, 6], [1, 3, 5, 7]];
            const reps = Math.max(1, Math.ceil(4 * N.box / (40 * boxes.length)));
            for (const c of Array(reps).fill(boxes).flat()) {
                const ctr = mul(c.reduce(add), 1 / 8);
                const targets = c.slice();
                for (const [a, b] of EDGES) targets.push(mul(add(c[a], c[b]), 0.5));
                for (const f of FACES) targets.push(mul(f.map(i => c[i]).reduce(add), 0.25));
                const axes = [sub(c[1], c[0]), sub(c[2], c[0]), sub(c[4], c[0])];
                for (const T of targets) {
                    // from a random point, and along one of the box's own axes (grazing the feature)
                    const from = r() < 0.5 ? point() : add(T, mul(axes[ri(3)], (r() < 0.5 ? -1 : 1) * (1 + r())));
                    const d = sub(T.map(f32), from.map(f32));
                    rays.push(mk(from, r() < 0.5 ? d : unit(d)));
                    feat.push({ T, from });
                    if (r() < 0.5) rays.push(mk(T, sub(T, ctr)));     // starting on the feature, heading out
                }
                for (const [a, b] of sample(EDGES, 3)) {            // along an edge, from its start and from before it
                    const e = sub(c[b], c[a]);
                    rays.push(mk(r() < 0.5 ? c[a] : sub(c[a], e), r() < 0.5 ? e : unit(e)));
                }
                for (const f of sample(FACES, 2)) {                 // in a face plane: corner to the opposite corner
                    const e = sub(c[f[3]], c[f[0]]), o = r() < 0.5 ? c[f[0]] : sub(c[f[0]], mul(e, r()));
                    rays.push(mk(o, e));
                    rays.push(mk(mul(add(c[f[0]], c[f[1]]), 0.5), sub(c[f[2]], c[f[0]])));
                }
            }
            emit("box_features", balance(rays.map(x => [x]), N.box), STD);
        }
        // ---- tri_features
        const isBvh = tris.length > 0;
        if (isBvh) {
            const rays = [];
            const chosen = sample(tris, 200);
            for (const tr of Array(Math.ceil(60 / chosen.length)).fill(chosen).flat()) {
                const [a, b, c] = tr.p, nrm = unit(cross(sub(b, a), sub(c, a)));
                const size = Math.max(len(sub(b, a)), len(sub(c, a)));
                if (!(size > 0) || !nrm.every(isFinite)) continue;
                const targets = [a, b, c, mul(add(a, b), 0.5), mul(add(b, c), 0.5), mul(add(a, c), 0.5), mul(add(add(a, b), c), 1 / 3)];
                for (const T of targets)
                    for (const side of [1, -1]) {
                        const from = add(T, mul(nrm, side * size * (0.5 + r())));
                        const d = sub(T.map(f32), from.map(f32));
                        rays.push(mk(from, r() < 0.5 ? d : unit(d), tr.obj));
                        if (r() < 0.6) rays.push(mk(T, mul(nrm, side * (0.5 + r())), tr.obj));   // starting on it, along the normal
                        if (r() < 0.3) {                                                     // a hair outside the triangle
                            const T2 = add(T, mul(sub(T, targets[6]), 2 ** -(10 + ri(12))));
                            rays.push(mk(from, sub(T2.map(f32), from.map(f32)), tr.obj));
                        }
                    }
                rays.push(mk(sub(a, sub(b, a)), sub(b, a), tr.obj));                             // along an edge
                rays.push(mk(a, sub(mul(add(b, c), 0.5), a), tr.obj));                           // in the plane, from a vertex
                for (const T of targets.slice(0, 3)) feat.push({ T, from: add(T, mul(nrm, size)) });
            }
            const check = (e, T, O, A) => {
                if (e.transp) {
                    const other = O.filter((o, k) => o >= 0 && A[k] >= 0 && o != A[k]).length;
                    if (other < 20) throw new Error(`${name}/${e.name}: only ${other} rays hit another triangle than the one aimed at`);
                    e.hit_other = other;
                }
            };
            emit("tri_features", balance(rays.map(x => [x]), N.tri), STD, { aim: true, check });
        }
        // ---- scaled: tiny and huge directions, far origins
        {
            const rays = [];
            const pool = sample(feat, 6 * N.scaled);
            pool.forEach((f, k) => {
                const d = sub(f.T, f.from);
                if (k % 3 == 0) rays.push(mk(f.from, mul(unit(d), 1e-3)));
                else if (k % 3 == 1) rays.push(mk(f.from, mul(unit(d), 1e3)));
                else {
                    const u = r() < 0.5 ? unit(d) : dir(), far = sub(f.T, mul(u, 1e3 * extent));
                    rays.push(mk(far, r() < 0.5 ? u : sub(f.T.map(f32), far.map(f32))));
                }
            });
            const wc = box.getCorners().map(c => Array.from(c).slice(0, 3)), wctr = Array.from(box.center).slice(0, 3);
            for (const h of hits) {
                const o = Array.from(h.ray.origin), d = Array.from(h.ray.direction), k = r() < 0.5 ? 1e-3 : 1e3;
                rays.push(mk(o, mul(d, k)));
                rays.push(mk(o, mul(d, -k)));                         // away from the hit
                // from far away, just past a corner of the scene's finite bounding box
                const c = wc[ri(8)], T = add(c, mul(sub(c, wctr), 1e-3 * r())), u = dir(), far = sub(T, mul(u, 1e3 * extent));
                rays.push(mk(far, r() < 0.5 ? u : sub(T.map(f32), far.map(f32))));
            }
            emit("scaled", balance(rays.map(x => [x]), N.scaled), STD);
        }

        const sha = crypto.createHash("sha256").update(blob).digest("hex");
        fs.writeFileSync(path.join(outdir, name + ".json"), JSON.stringify({ scene: name, blob_sha256: sha, bvh: isBvh, sets }));
        console.log(`${name}: ${sets.map(x => `${x.name} ${x.hits}/${x.n}` + (x.dropped ? ` (-${x.dropped})` : "")).join(", ")}`);
    }
}
main().catch(e => { console.error(e); process.exit(1); });
