"use strict";
/*
 * TEST INFRASTRUCTURE ONLY.  The "SDF zoo": small scenes of this project's own whose SDF trees lie outside the
 * shapes of the reference's seven SDF test scenes, so that none of their roots is a recognised program form
 * (jsraytracer_amd/csrc/sdf_program.h SFORM_*) and every one runs the device's program VM.  The trees are built at
 * run time from the reference's classes (load_reference.js refClass); the reference then computes the known
 * answers (regen_zoo.sh).
 *
 * Every scene: one camera (aspect 28:20, the thumbnail the fixtures render), a checkerboard floor plane at
 * y = -1, one point light, one small area light, and SDFGeometry(root, 128, 1e-4, 100) primitives.
 * `path` scenes use PhongPathTracingMaterial (rendered with the multisampling renderer), the others PhongMaterial
 * (rendered with SimpleRenderer).
 *
 *   scenes[name]() -> {renderer, width, height}, as a reference tests/<name>/test.mjs configureTest hands over.
 */
const { refClass } = require("./load_reference");

const C = (n) => refClass(n);
const V = (...a) => C("Vec").of(...a);
const M = () => C("Mat4");
const T = (x, y, z) => M().translation([x, y, z]);
const mk = (cls, ...a) => new (C(cls))(...a);
const matrix = (m) => mk("SDFMatrixTransformer", m);
const tx = (sdf, m) => mk("TransformSDF", sdf, matrix(m));

function sdfPrim(root, transform, path) {
    const material = path ? mk("PhongPathTracingMaterial", V(1, 1, 1), 0, 0.6, 0.3, 20)
                          : mk("PhongMaterial", V(1, 1, 1), 0.2, 0.4, 0.6, 100, 0.3);
    return mk("Primitive", mk("SDFGeometry", root, 128, 1e-4, 100), material, transform);
}

function scene(objects, camT, path) {
    const checker = mk("CheckerboardMaterialColor", V(1, 1, 1), V(0.1, 0.1, 0.1));
    const floor = mk("Primitive", mk("Plane"),
                     path ? mk("PhongPathTracingMaterial", checker, 0, 0.5, 0.2, 10)
                          : mk("PhongMaterial", checker, 0.1, 0.4, 0.6, 100, 0.3),
                     T(0, -1, 0).times(M().rotation(Math.PI / 2, V(1, 0, 0))));
    const lights = [
        mk("SimplePointLight", V(6, 8, 7, 1), V(1, 1, 1), 1500),
        mk("RandomSampleAreaLight", mk("Square"),
           T(-3, 7, 2).times(M().rotation(-Math.PI / 2, V(1, 0, 0))).times(M().scale([0.5, 0.5, 1])),
           V(1, 0.9, 0.8), 900, 1)];
    const camera = mk("PerspectiveCamera", Math.PI / 4, 28 / 20, camT);
    const world = mk("World", [floor].concat(objects), lights);
    return { renderer: path ? mk("IncrementalMultisamplingRenderer", world, camera, 2, 4)
                            : mk("SimpleRenderer", world, camera, 4),
             width: 28, height: 20 };
}

const lookAt = (x, y, z, yaw, pitch) => T(x, y, z).times(M().rotation(yaw, V(0, 1, 0))).times(M().rotation(pitch, V(1, 0, 0)));

// ---- the trees ----
// Round(Intersection(Box, Transform(Sphere, Matrix), Transform(Tetrahedron, Matrix)), 0.1):
// SOP_SUBK, SOP_MAX of three operands, indexOfMax over three children
function roundNary() {
    return mk("RoundSDF",
              mk("IntersectionSDF",
                 mk("BoxSDF", V(0.8, 0.7, 0.75), V(0.9, 0.2, 0.2)),
                 tx(mk("SphereSDF", 1.0, V(0.2, 0.9, 0.2)), T(0.15, 0.1, -0.05)),
                 tx(mk("TetrahedronSDF", V(0.2, 0.3, 0.9)), T(0, 0.05, 0).times(M().rotation(0.4, V(0, 1, 0))).times(M().scale(1.25)))),
              0.1);
}

// Union of six children of mixed kinds (SDF_MAX_D exactly); children 1 and 2 are the same sphere in two
// colours: equal distances everywhere, so getMaterialData must take the first (indexOfMin, math.js:53-70)
function unionWide() {
    const twin = T(0.9, 0.3, 0.2);
    return mk("UnionSDF",
              mk("BoxSDF", V(0.45, 0.6, 0.45), V(0.9, 0.8, 0.1)),
              tx(mk("SphereSDF", 0.55, V(1, 0.1, 0.1)), twin),
              tx(mk("SphereSDF", 0.55, V(0.1, 1, 0.1)), twin),
              tx(mk("TetrahedronSDF", V(0.1, 0.4, 1)), T(-1.1, 0, 0.1).times(M().scale(0.6))),
              mk("RoundSDF", tx(mk("BoxSDF", V(0.3, 0.2, 0.5), V(0.8, 0.3, 0.8)), T(0, 0.95, 0).times(M().rotation(0.5, V(0, 0, 1)))), 0.07),
              tx(mk("SphereSDF", 0.5, V(0.2, 0.9, 0.9)), T(-0.4, -0.2, 0.9).times(M().scale([1.3, 0.7, 1]))));
}

// Transform(Transform(Union(Box, Sphere), Sequence(Sequence(Matrix(rotation x non-uniform scale)), Reflection,
// Repetition(3, 0.7, 5))), Matrix(scale 2)): P-stack depth 2, scale-stack depth SDF_MAX_S (the inner Sequence
// around the Matrix is what takes it from 3 to 4), XREF / XREP outside a form, and sizes that are no powers of
// two (sdf_rep1's division)
function nestedTx() {
    const inner = mk("UnionSDF", mk("BoxSDF", V(0.3, 0.25, 0.35), V(0.9, 0.5, 0.1)), mk("SphereSDF", 0.38, V(0.1, 0.5, 0.9)));
    const seq = mk("SDFTransformerSequence",
                   mk("SDFTransformerSequence", matrix(M().rotation(0.3, V(0, 0, 1)).times(M().scale([1.2, 0.8, 1])))),
                   mk("SDFReflectionTransformer", V(1, 0.5, 0), 0.05),
                   mk("SDFInfiniteRepetitionTransformer", V(3, 0.7, 5)));
    return mk("TransformSDF", mk("TransformSDF", inner, seq), matrix(M().scale(2)));
}

// RecursiveTransformUnion(Sphere, Recursive(Sequence(Matrix, Reflection), 2), 3): two nested loops.  (With one
// more Sequence around the Recursive the scale stack would be 5 deep, one past SDF_MAX_S: the loader refuses
// that tree, tests/test_oracle_sdfzoo.py.)
function loops() {
    const step = mk("SDFTransformerSequence",
                    matrix(T(0.45, 0.3, 0.1).times(M().rotation(0.5, V(0, 1, 0.3))).times(M().scale(0.8))),
                    mk("SDFReflectionTransformer", V(0.2, 1, 0.1), -0.1));
    return mk("RecursiveTransformUnionSDF", mk("SphereSDF", 0.5, V(0.9, 0.6, 0.2)),
              mk("SDFRecursiveTransformer", step, 2), 3);
}
// zero iterations: the `ia <= 0` loop skip, in a union loop and in a transformer loop
const loopZeroUnion = () => mk("RecursiveTransformUnionSDF", mk("BoxSDF", V(0.4, 0.3, 0.4), V(0.3, 0.8, 0.3)),
                               matrix(T(0.5, 0, 0).times(M().scale(0.5))), 0);
const loopZeroTx = () => mk("TransformSDF", mk("SphereSDF", 0.45, V(0.3, 0.3, 0.9)),
                            mk("SDFRecursiveTransformer", matrix(M().scale(0.5)), 0));

// left-nested smooth combinators `depth` deep, cycling SmoothDifference / SmoothUnion / SmoothIntersection (the
// outermost of eight is a SmoothUnion) over spheres (UV) and boxes (no UV) of distinct colours: the distance stack
// stays at 2, the blend stack fills.  Every k is wide against the leaves' spacing and the intersections' operands
// are barely larger than the chain, so on most of the surface every level's mix factor lies strictly between 0
// and 1 and the colour of a hit depends on all the pending blends below it.
function smoothChain(depth) {
    const col = (i) => V(0.15 + 0.1 * i, 0.95 - 0.09 * i, (i % 3) * 0.4 + 0.1);
    const at = (i, r) => T(r * Math.cos(0.9 * i), 0.08 * (i % 3), r * Math.sin(0.9 * i));
    const leaf = (i) => (i % 2 === 0) ? tx(mk("SphereSDF", 0.5 + 0.02 * i, col(i)), at(i, 0.35))
                                      : tx(mk("BoxSDF", V(0.4, 0.32 + 0.02 * i, 0.36), col(i)), at(i, 0.3));
    let root = leaf(0);
    for (let i = 1; i <= depth; ++i) {
        const kind = (i + 1) % 3, k = 0.7 + 0.06 * (i % 4);
        if (kind === 0) root = mk("SmoothUnionSDF", root, leaf(i), k);
        else if (kind === 1)  // an operand barely larger than the chain
            root = mk("SmoothIntersectionSDF", root, (i % 2 === 0) ? tx(mk("SphereSDF", 0.85, col(i)), at(i, 0.1))
                                                                  : tx(mk("BoxSDF", V(0.8, 0.6, 0.75), col(i)), at(i, 0.1)), k);
        else  // a bite off the side
            root = mk("SmoothDifferenceSDF", root, (i % 2 === 0) ? tx(mk("SphereSDF", 0.3, col(i)), at(i, 0.85))
                                                                : tx(mk("BoxSDF", 0.25, col(i)), at(i, 0.85)), k);
    }
    return root;
}
// right-nested five deep: six distances on the stack at once (SDF_MAX_D)
function smoothRight() {
    const leaf = (i) => (i % 2 === 0)
        ? tx(mk("SphereSDF", 0.3, V(0.9 - 0.15 * i, 0.2 + 0.1 * i, 0.3)), T(-1 + 0.4 * i, 0.1 * (i % 2), 0))
        : tx(mk("BoxSDF", V(0.22, 0.3, 0.22), V(0.2, 0.3 + 0.1 * i, 0.9)), T(-1 + 0.4 * i, 0.1, 0.1));
    let root = leaf(5);
    for (let i = 4; i >= 0; --i) root = mk("SmoothUnionSDF", leaf(i), root, 0.2 + 0.03 * i);
    return root;
}

// a recognised form: the reference's Menger sponge shape, two levels (SFORM_RUNION_DIFF)
function menger2() {
    const s = 1 / 3;
    return mk("DifferenceSDF", mk("BoxSDF", 1),
              mk("RecursiveTransformUnionSDF",
                 mk("UnionSDF", mk("BoxSDF", V(Infinity, s, s)), mk("BoxSDF", V(s, Infinity, s)), mk("BoxSDF", V(s, s, Infinity))),
                 mk("SDFTransformerSequence", matrix(M().scale(s)), mk("SDFInfiniteRepetitionTransformer", V(2, 2, 2))),
                 2));
}

const scenes = {
    zoo_round_nary: () => scene([sdfPrim(roundNary(), T(0, 0, 0).times(M().rotation(0.3, V(0, 1, 0))), false)],
                                lookAt(0, 1.0, 3.1, 0, -0.25), false),
    zoo_union_wide: () => scene([sdfPrim(unionWide(), T(0, -0.2, 0), false)], lookAt(0, 1.1, 3.5, 0, -0.25), false),
    zoo_nested_tx: () => scene([sdfPrim(nestedTx(), T(0, 0.3, 0), false)], lookAt(0.5, 2.2, 9, 0, -0.2), false),
    zoo_loops: () => scene([sdfPrim(loops(), T(-0.3, 0, 0), false),
                            sdfPrim(loopZeroUnion(), T(-1.45, -0.5, 0.7), false),
                            sdfPrim(loopZeroTx(), T(1.35, -0.4, 0.8), false)],
                           lookAt(0, 0.9, 2.9, 0, -0.25), false),
    zoo_smooth_chain: () => scene([sdfPrim(smoothChain(8), T(-0.9, 0, 0), true),
                                   sdfPrim(smoothRight(), T(1.7, -0.3, 0.4).times(M().rotation(-0.4, V(0, 1, 0))), true)],
                                  lookAt(0.3, 1.2, 3.4, 0, -0.27), true),
    zoo_mixed: () => scene([sdfPrim(menger2(), T(-2.2, 0, -0.5).times(M().rotationY(0.5)), true),
                            sdfPrim(roundNary(), T(0, -0.1, 0.3), true),
                            sdfPrim(loops(), T(2.0, 0, -0.4), true),
                            mk("Primitive", mk("Sphere"), mk("PhongPathTracingMaterial", V(0.9, 0.3, 0.3), 0, 0.5, 0.4, 30),
                               T(0.9, -0.55, 1.9).times(M().scale(0.45))),
                            mk("Aggregate", [sdfPrim(unionWide(), T(0, 0, 0), true)],
                               T(-0.6, 1.9, -1.6).times(M().rotation(0.6, V(0, 1, 0))).times(M().scale(0.8)))],
                           lookAt(0.2, 1.6, 4.6, 0, -0.25), true),
};

module.exports = { scenes, smoothChain };
