"use strict";
/*
 * TEST INFRASTRUCTURE ONLY.  The "shading zoo": small scenes of this project's own that construct the materials
 * and lights the loader accepts and the kernels implement but none of the reference's own test scenes uses --
 * SolidColorMaterial, TransparentMaterial, two-child PhongMaterial, the Fresnel edge ratios, PhongPathTracingMaterial
 * scatter with a mirror probability strictly between 0 and 1, Circle and transformed Sphere area lights, light
 * colours that read UV.  Everything is built at run time from the reference's classes (load_reference.js refClass);
 * the reference then computes the known answers (regen_shadezoo.sh).  tests/test_oracle_shadezoo.py lists which
 * scene reaches which branch, and names the objects below by their OBJS index (the order they are listed in).
 *
 *   scenes[name]() -> {renderer, width, height}, as a reference tests/<name>/test.mjs configureTest hands over.
 */
const { refClass } = require("./load_reference");

const C = (n) => refClass(n);
const V = (...a) => C("Vec").of(...a);
const M = () => C("Mat4");
const T = (x, y, z) => M().translation([x, y, z]);
const S = (...s) => M().scale(s.length === 1 ? s[0] : s);
const R = (a, x, y, z) => M().rotation(a, V(x, y, z));
const mk = (cls, ...a) => new (C(cls))(...a);
const prim = (geom, material, transform, casts = true) =>
    mk("Primitive", typeof geom === "string" ? mk(geom) : geom, material, transform, M().inverse(transform), casts);
const checker = (a, b) => mk("CheckerboardMaterialColor", a, b);
const lookAt = (x, y, z, yaw, pitch) => T(x, y, z).times(R(yaw, 0, 1, 0)).times(R(pitch, 1, 0, 0));
const FLOOR_T = () => T(0, -1, 0).times(R(Math.PI / 2, 1, 0, 0));

const phongFloor = () => prim("Plane", mk("PhongMaterial", checker(V(1, 1, 1), V(0.1, 0.1, 0.1)), 0.1, 0.4, 0.6, 100, 0.3), FLOOR_T());
const pathFloor = () => prim("Plane", mk("PhongPathTracingMaterial", checker(V(1, 1, 1), V(0.1, 0.1, 0.1)), 0, 0.5, 0.2, 10), FLOOR_T());
const pointLight = () => mk("SimplePointLight", V(6, 8, 7, 1), V(1, 1, 1), 1500);
const squareLight = () => mk("RandomSampleAreaLight", mk("Square"), T(-3, 7, 2).times(R(-Math.PI / 2, 1, 0, 0)).times(S(0.5, 0.5, 1)),
                             V(1, 0.9, 0.8), 900, 1);

function simple(objects, lights, camT, depth, bg) {
    const world = bg ? mk("World", objects, lights, bg) : mk("World", objects, lights);
    return { renderer: mk("SimpleRenderer", world, mk("PerspectiveCamera", Math.PI / 4, 28 / 20, camT), depth), width: 28, height: 20 };
}
function path(objects, lights, camT, depth) {
    return { renderer: mk("IncrementalMultisamplingRenderer", mk("World", objects, lights),
                          mk("PerspectiveCamera", Math.PI / 4, 28 / 20, camT), 3, depth), width: 28, height: 20 };
}

// ---- the materials shz_profiles repeats on every kind of primitive ----
const solidM = () => mk("SolidColorMaterial", V(0.2, 0.7, 0.9));
const transparentM = () => mk("TransparentMaterial", V(0.9, 0.4, 0.2), 0.35);
const twoChildM = () => mk("PhongMaterial", V(0.9, 0.8, 0.3), 0.1, 0.4, 0.5, 40, 0.3, 0.4);
const fresnel075M = () => mk("FresnelPhongMaterial", V(0.5, 0.9, 0.6), 0.05, 0.3, 0.4, 30, 0.75);

// Triangle primitives side by side (up, down, up, down), one material each, under a BVH built as the
// reference's hollow-tetrahedron scene builds its own (BVHAggregate.build(triangles, transform))
function triangleBvh(materials, transform) {
    const tris = materials.map((m, i) => {
        const x = -2.25 + 1.5 * i, y = i % 2 ? -0.7 : 0.7;
        return mk("Primitive", mk("Triangle", [V(x - 1.1, -y, 0, 1), V(x + 1.1, -y, 0, 1), V(x, y, 0, 1)]), m);
    });
    return C("BVHAggregate").build(tris, transform);
}

const sdf = (root, material, t) => prim(mk("SDFGeometry", root, 128, 1e-4, 100), material, t);
const profileMaterials = () => [solidM(), transparentM(), twoChildM(), fresnel075M()];
const profileLights = () => [
    mk("RandomSampleAreaLight", mk("Circle"), T(0, 6, 4).times(R(-1.2, 1, 0, 0)).times(S(1.5, 0.8, 1)), V(1, 0.95, 0.9), 900, 2),
    mk("SimplePointLight", V(-5, 4, 6, 1), V(1, 1, 1), 500)];
const PX = [-2.25, -0.75, 0.75, 2.25];

const scenes = {
    // objects: 0 floor, 1 Solid (solid colour), 2 Solid (checkerboard colour, a Square: UV = local xy, four quadrants),
    // 3 Transparent 0.35, 4 Transparent 0 that casts no shadow, 5 Transparent 1, 6-9 four Transparent sheets one behind
    // the other (depth 4: the fourth sheet's child is cut), 10 Phong with transmissivity (the normalised direction)
    shz_solid_transparent: () => simple([
        phongFloor(),
        prim("Sphere", mk("SolidColorMaterial", V(0.2, 0.7, 0.9)), T(-2.5, 1.55, 0).times(S(0.8))),
        prim("Square", mk("SolidColorMaterial", checker(V(0.9, 0.2, 0.2), V(0.1, 0.9, 0.3))), T(-0.85, 1.55, 0).times(R(0.3, 0, 1, 0)).times(S(1.5))),
        prim("Sphere", mk("TransparentMaterial", V(0.9, 0.4, 0.2), 0.35), T(0.85, 1.55, 0).times(S(0.8))),
        prim("Sphere", mk("TransparentMaterial", V(0.3, 0.3, 0.9), 0), T(2.5, 1.55, 0).times(S(0.8)), false),
        prim("Square", mk("TransparentMaterial", checker(V(0.8, 0.8, 0.2), V(0.2, 0.2, 0.8)), 1), T(-2.5, -0.2, 0.3).times(R(-0.4, 1, 0, 0)).times(S(1.5))),
        prim("Square", mk("TransparentMaterial", V(0.9, 0.1, 0.1), 0.35), T(-0.85, -0.15, 0.9).times(S(1.5))),
        prim("Square", mk("TransparentMaterial", V(0.1, 0.9, 0.1), 0.35), T(-0.85, -0.15, 0.6).times(S(1.5))),
        prim("Square", mk("TransparentMaterial", V(0.1, 0.1, 0.9), 0.35), T(-0.85, -0.15, 0.3).times(S(1.5))),
        prim("Square", mk("TransparentMaterial", V(0.9, 0.9, 0.1), 0.35), T(-0.85, -0.15, 0.0).times(S(1.5))),
        prim("Sphere", mk("PhongMaterial", V(0.8, 0.8, 0.9), 0.1, 0.3, 0.5, 50, 0, 0.6), T(1.6, -0.25, 0.5).times(S(0.8))),
    ], [pointLight(), squareLight()], lookAt(0, 0.9, 6.8, 0, -0.04), 4),

    // objects: 0 floor, 1 back wall with a checkerboard reflectivity whose second colour is black (and a
    // transmissivity: one or two children by the hit's UV), 2 reflectivity and transmissivity, 3 vector reflectivity,
    // 4 reflectivity scaled per channel and transmissivity, 5 smoothness 0, 6 smoothness 1e6 with specularity 0,
    // 7 specularity 0 with ambient
    shz_phong_children: () => simple([
        phongFloor(),
        prim("Square", mk("PhongMaterial", V(0.6, 0.7, 0.9), 0.15, 0.3, 0.2, 20, checker(V(0.5, 0.5, 0.5), V(0, 0, 0)), 0.25),
             T(0, 0.6, -2).times(R(0.35, 0, 1, 0)).times(S(7, 3.2, 1))),
        prim("Sphere", mk("PhongMaterial", V(0.9, 0.8, 0.3), 0.1, 0.4, 0.5, 40, 0.3, 0.4), T(-2.1, 1.5, 0).times(S(0.75))),
        prim("Sphere", mk("PhongMaterial", V(0.9, 0.9, 0.9), 0.05, 0.3, 0.4, 60, V(0.7, 0.35, 0.1)), T(0, 1.5, 0).times(S(0.75))),
        prim("Sphere", mk("PhongMaterial", V(0.4, 0.9, 0.5), 0.1, 0.3, 0.3, 30, [0.125, 0.5, 0.25], [0.5, 0.25, 0.375]), T(2.1, 1.5, 0).times(S(0.75))),
        prim("Sphere", mk("PhongMaterial", V(0.9, 0.3, 0.3), 0.1, 0.4, 0.5, 0), T(-2.1, -0.2, 0.6).times(S(0.75))),
        prim("Sphere", mk("PhongMaterial", V(0.3, 0.4, 0.9), 0.1, 0.6, 0, 1e6), T(0, -0.2, 0.6).times(S(0.75))),
        prim("Sphere", mk("PhongMaterial", V(0.8, 0.5, 0.9), 0.3, 0.5, 0, 100), T(2.1, -0.2, 0.6).times(S(0.75))),
    ], [pointLight(), squareLight()], lookAt(0, 0.8, 7.0, 0, -0.03), 5),

    // objects: 0 floor, 1 ratio 0.75, 2 ratio 1, 3 ratio 1.5 with light 1 inside it, 4 ratio Infinity, 5 a ratio-1.5
    // pane whose normal points away from the camera (backside primary hits, many past the critical angle)
    shz_fresnel_edges: () => simple([
        phongFloor(),
        prim("Sphere", mk("FresnelPhongMaterial", V(0.5, 0.9, 0.6), 0.05, 0.3, 0.4, 30, 0.75), T(-2.4, 0.1, 0).times(S(1.0))),
        prim("Sphere", mk("FresnelPhongMaterial", V(0.9, 0.6, 0.5), 0.05, 0.3, 0.4, 30, 1.0), T(-0.1, 1.5, -0.5).times(S(0.9))),
        prim("Sphere", mk("FresnelPhongMaterial", V(0.6, 0.6, 0.95), 0.05, 0.3, 0.4, 30, 1.5), T(0.2, -0.1, 1.0).times(S(0.9))),
        prim("Sphere", mk("FresnelPhongMaterial", V(0.9, 0.9, 0.4), 0.05, 0.3, 0.4, 30, Infinity), T(2.6, 0.0, 0).times(S(0.95))),
        prim("Square", mk("FresnelPhongMaterial", V(0.7, 0.9, 0.9), 0.05, 0.3, 0.4, 30, 1.5),
             T(2.3, 1.9, 0.5).times(R(Math.PI - 1.08, 0, 1, 0)).times(S(2.4, 1.3, 1))),
    ], [pointLight(), mk("SimplePointLight", V(0.2, 0.15, 1.1, 1), V(1, 0.8, 0.6), 12)], lookAt(0.3, 1.0, 7.0, 0, -0.08), 6),

    // objects: 0 floor, 1 mirror probability 0.3 with ratio Infinity, 2 mirror probability 0.5 with ratio 1.5,
    // 3 diffusivity = specularity = 0 with mirror probability 0.5 (probSum == 0: no child after one draw),
    // 4 specular only, 5 diffusivity = specularity = 0 with ratio 1.5 (both scatters may end the path)
    shz_path_scatter: () => path([
        pathFloor(),
        prim("Sphere", mk("PhongPathTracingMaterial", V(0.9, 0.5, 0.3), 0, 0.5, 0.3, 20, Infinity, 0.3), T(-2.3, 1.45, 0).times(S(0.8))),
        prim("Sphere", mk("PhongPathTracingMaterial", V(0.5, 0.8, 0.9), 0, 0.3, 0.3, 25, 1.5, 0.5), T(0, 1.45, 0).times(S(0.8))),
        prim("Sphere", mk("PhongPathTracingMaterial", V(0.9, 0.9, 0.9), 0.2, 0, 0, 10, Infinity, 0.5), T(2.3, 1.45, 0).times(S(0.8))),
        prim("Sphere", mk("PhongPathTracingMaterial", V(0.8, 0.9, 0.4), 0, 0, 0.6, 40), T(-1.2, -0.2, 0.8).times(S(0.8))),
        prim("Sphere", mk("PhongPathTracingMaterial", V(0.9, 0.6, 0.9), 0.1, 0, 0, 10, 1.5, 0.5), T(1.2, -0.2, 0.8).times(S(0.8))),
    ], [pointLight(), squareLight()], lookAt(0, 0.8, 7.0, 0, -0.03), 5),

    // lights: 0 point light with a checkerboard colour (UV = cartesianToSpherical of the direction), 1 Sphere light
    // under rotation x non-uniform scale with a checkerboard colour (UV of the picked normal), samples 2, 2 rotated
    // Square light whose checkerboard colour sits in a per-channel ScaledMaterialColor (UV = local xy: all four
    // quadrants are drawn)
    shz_light_uv: () => simple([
        phongFloor(),
        prim("Sphere", mk("PhongMaterial", V(0.9, 0.9, 0.9), 0.05, 0.6, 0.4, 30), T(-1.5, -0.2, 0).times(S(0.8))),
        prim("Sphere", mk("PhongMaterial", V(0.9, 0.6, 0.4), 0.05, 0.6, 0.4, 30, 0.2), T(1.4, -0.3, 0.6).times(S(0.7))),
    ], [
        mk("SimplePointLight", V(4, 3, 5, 1), checker(V(1, 0.9, 0.7), V(0, 0.2, 1)), 300),
        mk("RandomSampleAreaLight", mk("Sphere"), T(-3, 2.5, 1).times(R(0.7, 1, 0.4, 0.2)).times(S(0.9, 0.3, 0.5)),
           checker(V(0.6, 1, 0.7), V(1, 0, 0.3)), 250, 2),
        mk("RandomSampleAreaLight", mk("Square"), T(0.3, 2.2, -0.5).times(R(-1.2, 1, 0, 0.3)).times(S(2.5, 2.5, 1)),
           mk("ScaledMaterialColor", checker(V(1, 1, 0.2), V(0.1, 0.2, 1)), [1, 0.75, 0.5]), 160, 1),
    ], lookAt(0, 1.4, 6.0, 0, -0.3), 4),

    // lights: 0 Circle under rotation x non-uniform scale, samples 3, 1 Square, samples 2, 2 Sphere, samples 1,
    // 3 point light, 4 point light below the floor (every lit surface shows it its backside or is shadowed by the
    // floor).  objects: 0 floor, 1 sphere, 2 a sheet between the lights and the floor that casts no shadow, 3 sphere
    shz_light_mix: () => simple([
        phongFloor(),
        prim("Sphere", mk("PhongMaterial", V(0.9, 0.9, 0.9), 0.05, 0.6, 0.4, 30, 0.2), T(-1.6, -0.2, 0).times(S(0.8))),
        prim("Square", mk("PhongMaterial", V(0.9, 0.3, 0.3), 0.1, 0.6, 0.3, 20), T(0.2, 0.3, 0.8).times(R(-Math.PI / 2 + 0.5, 1, 0, 0)).times(S(2.2, 1.6, 1)), false),
        prim("Sphere", mk("PhongMaterial", V(0.4, 0.6, 0.9), 0.05, 0.6, 0.4, 30), T(1.7, -0.3, -0.4).times(S(0.7))),
    ], [
        mk("RandomSampleAreaLight", mk("Circle"), T(0.5, 3.0, 0.5).times(R(-1.3, 1, 0.2, 0)).times(S(1.6, 0.6, 1)), V(1, 0.95, 0.8), 260, 3),
        mk("RandomSampleAreaLight", mk("Square"), T(-3, 2.5, 2).times(R(-Math.PI / 2, 1, 0, 0)).times(S(0.8, 0.8, 1)), V(0.6, 0.8, 1), 200, 2),
        mk("RandomSampleAreaLight", mk("Sphere"), T(3, 2.0, 1.5).times(S(0.3)), V(1, 0.6, 0.5), 150, 1),
        mk("SimplePointLight", V(-1, 4, 5, 1), V(1, 1, 1), 200),
        mk("SimplePointLight", V(0.5, -2.5, 0.5, 1), V(0.5, 1, 0.5), 400),
    ], lookAt(0, 1.6, 6.2, 0, -0.3), 4, V(0.15, 0.2, 0.35)),

    // the Solid, Transparent, two-child Phong and Fresnel ratio-0.75 materials (objects 1-4) on SDFGeometry primitives
    // alone (the SDF profile); a Circle light and a point light, as in the two scenes below
    shz_profiles_sdf: () => {
        const m = profileMaterials();
        return simple([
            phongFloor(),
            sdf(mk("SphereSDF", 0.68, V(0.9, 0.9, 0.3)), m[0], T(PX[0], 0.3, 0)),
            sdf(mk("BoxSDF", V(0.55, 0.55, 0.3), V(0.9, 0.5, 0.9)), m[1], T(PX[1], 0.3, 0).times(R(0.4, 0, 1, 0))),
            sdf(mk("SphereSDF", 0.68, V(0.6, 0.9, 0.9)), m[2], T(PX[2], 0.3, 0)),
            sdf(mk("RoundSDF", mk("BoxSDF", V(0.42, 0.42, 0.42), V(0.9, 0.9, 0.9)), 0.15), m[3], T(PX[3], 0.3, 0).times(R(0.5, 0.3, 1, 0))),
        ], profileLights(), lookAt(0, 0.8, 5.9, 0, -0.1), 5);
    },
    // ... on the triangles 1-4 of the BVH 5 alone (the mesh profile)
    shz_profiles_mesh: () => simple([phongFloor(), triangleBvh(profileMaterials(), T(0, 0.3, 0.3).times(R(0.15, 1, 0, 0)))],
                                    profileLights(), lookAt(0, 0.8, 5.9, 0, -0.1), 5),
    // ... on the children 1-4 of the Aggregate 5, beside an SDFGeometry primitive 6 (Transparent) and the BVH 9 of
    // two triangles 7-8 (Solid, Fresnel): every feature at once
    shz_profiles_all: () => {
        const m = profileMaterials();
        return simple([
            phongFloor(),
            mk("Aggregate", [
                prim("Sphere", m[0], T(PX[0], 0, 0).times(S(0.68))),
                prim("Square", m[1], T(PX[1], 0, 0).times(S(1.25))),
                prim("Sphere", m[2], T(PX[2], 0, 0).times(S(0.68))),
                prim("Sphere", m[3], T(PX[3], 0, 0).times(R(0.6, 0, 0, 1)).times(S(0.7, 0.75, 0.5))),
            ], T(0, 0.1, 0.2).times(R(0.1, 0, 1, 0)).times(S(1, 1.05, 1))),
            sdf(mk("BoxSDF", V(0.55, 0.55, 0.3), V(0.9, 0.5, 0.9)), transparentM(), T(-1.6, 1.7, 0).times(R(0.4, 0, 1, 0))),
            triangleBvh([solidM(), fresnel075M()], T(2.6, 1.7, 0.3).times(R(0.15, 1, 0, 0)).times(S(0.9))),
        ], profileLights(), lookAt(0, 0.9, 5.9, 0, -0.03), 5);
    },
};

module.exports = { scenes };
