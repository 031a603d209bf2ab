// Host build of the shadow cast's origin / direction split (jsraytracer_amd/csrc/device_common.h
// prim_local_origin + prim_any_local, root_slab + root_needed_at) for tests/test_shadow_split.py: the split
// form's distance and cull decision against the unsplit ones (prim_any's branches, root_needed), bit for bit.
#include "../../jsraytracer_amd/csrc/device_common.h"

// prims: n DPrim-like rows of 12 doubles (inv rows 0..2) + kinds[i] + boxes n x 6 floats (center, half);
// rays n x 6 floats (world o, d).  t_unsplit[i]: the distance as prim_any reads it; t_split[i]: through the
// local origin computed on its own.
extern "C" void split_any(const double *inv, const int *kinds, const float *boxes, const float *rays, long n,
                          double minD, double maxD, double *t_unsplit, double *t_split) {
    using namespace jsrt;
    for (long i = 0; i < n; ++i) {
        const float *r = rays + 6 * i;
        const F3 o = f3(r[0], r[1], r[2]), d = f3(r[3], r[4], r[5]);
        DPrim P{};
        for (int k = 0; k < 12; ++k) P.inv[k] = inv[12 * i + k];
        for (int k = 0; k < 3; ++k) {
            P.center[k] = boxes[6 * i + k];
            P.half[k] = boxes[6 * i + 3 + k];
        }
        P.gkind = kinds[i];
        P.casts_shadow = 1;
        // prim_any's branches, as written there
        const int k = P.gkind;
        double t = 0, u = 0;
        if (k == JSRT_GEOM_AABB) {
            const F3 lo = xf_point(P.inv, o), ld = xf_dir(P.inv, d);
            const int dec = box_any_f32(P.center, P.half, lo, box_ray(ld), minD, maxD, t);
            u = dec >= 0 ? (dec ? t : -DINF) : aabb_intersect(P.center, P.half, lo, ld, minD, maxD);
        } else if (k == JSRT_GEOM_PLANE || k == JSRT_GEOM_SQUARE || k == JSRT_GEOM_CIRCLE) {
            const int dec = planar_any_f32(k, P.inv, o, d, minD, maxD, t);
            u = dec >= 0 ? (dec ? t : -DINF) : planar_intersect(k, P.inv, o, d, minD, maxD);
        } else {
            const F3 lo = xf_point(P.inv, o), ld = xf_dir(P.inv, d);
            const int dec = sphere_any_f32(lo, ld, minD, maxD, t);
            u = dec >= 0 ? (dec ? t : -DINF) : sphere_static(lo, ld, minD);
        }
        t_unsplit[i] = u;
        double v = 0;
        const bool handled = prim_any_local(P, o, prim_local_origin(P, o), d, minD, maxD, v);
        t_split[i] = handled ? v : __builtin_nan("");
    }
}

// bounds: n x 8 floats (lo xyz, k, hi xyz, e0); rays n x 6 floats.  The cull's decision unsplit and split.
extern "C" void split_cull(const float *bounds, const float *rays, long n, double minD, double maxD, int *unsplit,
                           int *split) {
    using namespace jsrt;
    for (long i = 0; i < n; ++i) {
        const float *b = bounds + 8 * i, *r = rays + 6 * i;
        RootBound RB{};
        for (int k = 0; k < 3; ++k) {
            RB.lo[k] = b[k];
            RB.hi[k] = b[4 + k];
        }
        RB.k = b[3];
        RB.e0 = b[7];
        RB.bounded = 1;
        const F3 o = f3(r[0], r[1], r[2]);
        const float ix = 1.0f / r[3], iy = 1.0f / r[4], iz = 1.0f / r[5];
        const float oabs = fmaxf(fabsf(o.x), fmaxf(fabsf(o.y), fabsf(o.z)));
        unsplit[i] = root_needed(RB, o, ix, iy, iz, oabs, (float)minD, (float)maxD) ? 1 : 0;
        split[i] = root_needed_at(root_slab(RB, o, oabs), ix, iy, iz, (float)minD, (float)maxD) ? 1 : 0;
    }
}
