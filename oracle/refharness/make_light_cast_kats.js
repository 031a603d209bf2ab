"use strict";
/*
 * TEST INFRASTRUCTURE ONLY.  Shadow-segment known answers for World.cast, computed by the reference itself
 * (vm-loaded by load_reference.js), beside make_edge_cast_kats.js: the segments the render's shadow casts run,
 * from a reference hit point P to the sample points of the scene's lights -- the only segments the shadow-root
 * masks of the GPU's shadow grid hold for.  The directions are the `direction` the lights' own sampleIterator(P)
 * yields (lights.js:45-53, 80-92; Math.random is replaced by this file's generator while it runs), stored as
 * the f32 values the reference's Vec holds.
 *
 * One set, "to_light": minD 0.0001, maxD 1, shadow casters only (world.js:125-137).  Its rays come in groups of
 * 64 consecutive rays sharing an origin (the last group has 37: a ragged last wave), so that a wave of 64
 * consecutive rays lies in one cell of any spatial grid.  The groups are chosen so that the set has shadowed and
 * lit segments.
 *
 *   node oracle/refharness/make_light_cast_kats.js <outdir> <scene>...
 * writes <outdir>/<scene>.json in make_cast_kats.js's format, plus per set: kind, n, dropped, hits, group.
 */
const fs = require("fs");
const path = require("path");
const crypto = require("crypto");
const { loadScene, refClass } = require("./load_reference");
const { SceneBlobWriter } = require("../../jsraytracer_amd/js/scene_blob");

let s = 0x2468ace;
function r() { s = (Math.imul(s, 1103515245) + 12345) >>> 0; return s / 4294967296; }
const b64 = (typed) => Buffer.from(typed.buffer, typed.byteOffset, typed.byteLength).toString("base64");

const GROUP = 64, LAST = 37, CANDIDATES = 400;

async function main() {
    const argv = process.argv.slice(2);
    const outdir = path.resolve(argv[0]);
    fs.mkdirSync(outdir, { recursive: true });
    const Vec = refClass("Vec"), Ray = refClass("Ray");
    for (const name of argv.slice(1)) {
        const test = await loadScene(name);
        const w = new SceneBlobWriter();
        const blob = w.build(test);
        const world = test.renderer.world;
        const box = world.getFiniteBoundingBox();
        const point = () => [0, 1, 2].map(i => box.center[i] + 3 * box.half_size[i] * (r() - 0.5));
        const dir = () => { const th = 2 * Math.PI * r(), z = 2 * r() - 1, q = Math.sqrt(1 - z * z); return [q * Math.cos(th), q * Math.sin(th), z]; };
        const objOf = (o) => (o == null ? -1 : w.maps.obj.get(o));
        if (!world.lights.length) throw new Error(name + ": no lights");
        const area = world.lights.some(l => l.samples !== undefined);
        const groups_wanted = area ? 24 : 48;    // a point light's 64 segments are one segment: more origins instead

        // candidate groups: a reference hit point and 64 of the lights' samples from it
        const cands = [];
        const random = Math.random;
        Math.random = r;
        try {
            for (let k = 0; k < 20 * CANDIDATES && cands.length < CANDIDATES; ++k) {
                const p = point(), d = dir();
                const ray = new Ray(Vec.of(p[0], p[1], p[2], 1), Vec.of(d[0], d[1], d[2], 0));
                const h = world.cast(ray);
                if (h.object == null || !isFinite(h.distance) || !(h.distance > 0)) continue;
                const P = ray.getPoint(h.distance);
                if (!P.every(isFinite)) continue;
                const rays = [];
                while (rays.length < GROUP)
                    for (const light of world.lights)
                        for (const smp of light.sampleIterator(P))
                            if (rays.length < GROUP) rays.push(new Ray(P, smp.direction));
                if (!rays.every(x => x.direction.every(isFinite) && x.direction.slice(0, 3).some(c => c != 0))) continue;
                const res = rays.map(x => { const c = world.cast(x, 0.0001, 1, false); return { t: c.distance, obj: objOf(c.object) }; });
                cands.push({ rays, res, shadowed: res.filter(x => x.obj >= 0).length });
            }
        } finally {
            Math.random = random;
        }
        if (cands.length < groups_wanted) throw new Error(name + ": too few reference hits");
        // a third of the groups from the most shadowed origins, a third from the least, the rest as they came
        const picked = new Set(cands.slice(0, groups_wanted - 2 * Math.floor(groups_wanted / 3)));
        const rest = () => cands.filter(c => !picked.has(c));
        for (const c of rest().sort((a, b) => b.shadowed - a.shadowed).slice(0, Math.floor(groups_wanted / 3))) picked.add(c);
        for (const c of rest().sort((a, b) => a.shadowed - b.shadowed).slice(0, Math.floor(groups_wanted / 3))) picked.add(c);
        const groups = cands.filter(c => picked.has(c));
        // the ragged last wave is a group with shadowed and lit segments where there is one
        groups.sort((a, b) => (a.shadowed > 0 && a.shadowed < GROUP) - (b.shadowed > 0 && b.shadowed < GROUP));

        const all = [];
        groups.forEach((g, gi) => {
            const m = gi == groups.length - 1 ? LAST : GROUP;
            for (let k = 0; k < m; ++k) all.push({ ray: g.rays[k], ...g.res[k] });
        });
        const kept = all.filter(x => !Number.isNaN(x.t));
        const n = kept.length, dropped = all.length - n;
        if (dropped > 0) throw new Error(`${name}/to_light: ${dropped} rays are NaN in the reference (they would break the groups of 64)`);
        const R = new Float32Array(6 * n), T = new Float64Array(n), O = new Int32Array(n);
        kept.forEach((x, j) => {
            for (let i = 0; i < 3; ++i) { R[6 * j + i] = x.ray.origin[i]; R[6 * j + 3 + i] = x.ray.direction[i]; }
            T[j] = x.t; O[j] = x.obj;
        });
        const hits = O.reduce((acc, o) => acc + (o >= 0), 0);
        if (!(hits > 0 && hits < n)) throw new Error(`${name}/to_light: ${hits} shadowed segments of ${n}`);
        const sets = [{ name: "to_light", kind: "to_light", minD: 0.0001, maxD: 1, transp: false, n, dropped, hits, group: GROUP,
                        rays: b64(R), t: b64(T), obj: b64(O) }];
        const sha = crypto.createHash("sha256").update(blob).digest("hex");
        fs.writeFileSync(path.join(outdir, name + ".json"), JSON.stringify({ scene: name, blob_sha256: sha, sets }));
        console.log(`${name}: to_light ${hits}/${n} shadowed, ${groups.length} origins`);
    }
}
main().catch(e => { console.error(e); process.exit(1); });
